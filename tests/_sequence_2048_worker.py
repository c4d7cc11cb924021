"""The training step of tests/test_gpu_sequence_2048.py at max_sequence_length 2048: inputs() builds the configuration, parameters,
batch and masks (numpy only); run() does one forward + backward on the GPU.  As a program -- the RSYS_* switches are read once per
process, so a switched arm is a process of its own: python _sequence_2048_worker.py <out.npz> <dtype> <repository root>."""
import sys

import numpy as np

TASK_W = [0.05, 0.2, 0.3, 0.25]
GRADS = ("transformers.layers.0.attn.q_proj.weight", "transformers.layers.0.attn.v_proj.weight",
         "item_embedding.matchedid_embedding.embedding.weight")
ROWS, SEED, PAD = 2, 77, 37


def inputs():
    """hd64 narrowed to one layer at S = 2048: two rows; row 0 holds real users and ends in PAD padding interactions, row 1 is padding only"""
    from oracle import synth
    cfg = synth.make_config("hd64", mask_rate=0.15, mask_topk=320, max_sequence_length=2048, num_layers=1)
    P = synth.make_params(cfg, SEED, "test")
    d = synth.make_batch(cfg, ROWS, SEED + 1, mu=np.log(400.0), sigma=0.9)
    S = cfg["max_sequence_length"]
    for k in d:
        d[k][S - PAD:] = 0
    wm, rm = synth.make_masks(cfg, ROWS, SEED + 2)
    return cfg, P, d, wm, rm


def run(dtype):
    import recommendersystem_amd as ra
    cfg, P, d, wm, rm = inputs()
    model = ra.RecommenderModel(cfg, dtype=dtype, max_rows=ROWS)
    model.load_state_dict(P)
    model.set_loss_weights(TASK_W, 1)
    losses = model(d, False, masks=(wm, rm))
    out = {"losses": np.array(losses, np.float64), "trunk": np.array(model.trunk_output(ROWS))}
    for n in GRADS:
        out["g/" + n] = np.array(model.grad(n))
    model.close()
    return out


if __name__ == "__main__":
    out, dtype, root = sys.argv[1:4]
    sys.path.insert(0, root)
    np.savez(out, **run(dtype))
