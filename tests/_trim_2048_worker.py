"""The map-width edge of tests/test_gpu_trimmed_inference.py at max_sequence_length 2048, as a program of its own (like
_sequence_2048_worker.py): python _trim_2048_worker.py <out.npz> <dtype> <repository root>.  hd64 narrowed to one layer; a user of 1000
events (row_len 1024: 32 tiles, the 32-bit tile maps on arrays sized for the 64-bit ones) and one of 1030 (row_len 1056: 33 tiles, the
64-bit maps), each alone, trimmed and untrimmed: the retrieval embedding and the tokens either forward ran over."""
import os
import sys

import numpy as np


def run(dtype):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _trim_util as tu
    from recommendersystem_amd import serve
    cfg, V = tu.config(S=2048, num_layers=1)
    model, P, adapters = tu.make_model(cfg, "base", dtype, max_rows=1)
    rng = np.random.default_rng(21)
    out = {}
    for n in (1000, 1030):
        user = tu.user_with_history(rng, n, [], n_items=100)
        out[f"full_{n}"] = np.asarray(serve.predict(model, [user], "retrieval", 1)[0]["1.retrieval"], np.float32)
        out[f"tokens_full_{n}"] = np.int64(model.forward_tokens)
        out[f"trim_{n}"] = np.asarray(serve.predict(model, [user], "retrieval", 1, trim=True)[0]["1.retrieval"], np.float32)
        out[f"tokens_{n}"] = np.int64(model.forward_tokens)
    model.close()
    return out


if __name__ == "__main__":
    out, dtype, root = sys.argv[1:4]
    sys.path.insert(0, root)
    np.savez(out, **run(dtype))
