"""CPU: the host side of retrieval top-k -- the watched-item exclusions of Inference/render.jl:255-266 and serve.retrieve's argument
handling (checked before anything reaches the library)."""
import numpy as np
import pytest

from recommendersystem_amd import serve
from recommendersystem_amd.model import exclusion_csr


def _ev(medium, item, status):
    return {"medium": medium, "matchedid": item, "status": status}


def test_watched_exclusions_every_status():
    # statuses 0..8 (render.jl:13-23) on items 10..18 of both mediums; a later event overrides an earlier one
    items = [_ev(m, 10 + s, s) for m in (0, 1) for s in range(9)]
    items += [_ev(0, 30, 7), _ev(0, 30, 5),       # completed, then planned: kept
              _ev(1, 31, 5), _ev(1, 31, 6),       # planned, then watching: excluded
              _ev(0, 0, 5)]                       # item 0 is always excluded
    want = {0: [0, 10, 11, 12, 14, 16, 17, 18], 1: [0, 10, 11, 12, 14, 16, 17, 18, 31]}
    for m in (0, 1):
        got = serve.watched_exclusions(items, m)
        assert got.dtype == np.int32 and got.tolist() == want[m], (m, got)
    assert serve.watched_exclusions([], 1).tolist() == [0]


class _Stub:
    """A model that records the call instead of running it (no GPU here)."""
    def __init__(self):
        from oracle import synth
        self.config = synth.make_config("hd64")
        self.calls = []

    def retrieve_topk(self, q, medium, k, group=None, prior=None, exclude=None):
        self.calls.append((q, medium, k, group, prior, exclude))
        ng = q.shape[0] if group is None else int(np.max(group)) + 1
        ids = np.tile(np.arange(k, dtype=np.int32), (ng, 1))
        return ids, -np.ones((ng, k), np.float32), np.full(ng, k, np.int32)


def test_serve_retrieve_argument_handling():
    m = _Stub()
    D = m.config["embed_dim"]
    e = [{"0.retrieval": [0.0] * D} for _ in range(3)]
    bad = [
        dict(embeds=e, medium=0, k=5, groups=[0, 2, 2]),                 # group 1 has no embedding
        dict(embeds=e, medium=0, k=5, groups=[0, 1]),                    # one group id short
        dict(embeds=e, medium=0, k=5, groups=[0, -1, 1]),
        dict(embeds=e, medium=0, k=0),
        dict(embeds=e, medium=0, k=121),                                 # > V_0 = 120
        dict(embeds=e, medium=2, k=5),
        dict(embeds=e, medium=0, k=5, exclude=[[1], [2]]),               # 2 lists for 3 groups
        dict(embeds=e, medium=0, k=5, exclude=[[1], [120], []]),         # id out of range
        dict(embeds=e, medium=0, k=5, prior=np.zeros((3, 7), np.float32)),
        dict(embeds=[], medium=0, k=5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            serve.retrieve(m, **kw)
    assert not m.calls
    out = serve.retrieve(m, e, 0, 4, groups=[1, 0, 1], exclude=[[3], [1, 1, 7, 2]], coefs=[0.5])
    assert len(out) == 2 and len(m.calls) == 1
    q, medium, k, group, prior, exclude = m.calls[0]
    assert q.shape == (3, D) and medium == 0 and k == 4 and group.tolist() == [1, 0, 1]
    assert np.allclose(out[1][1], -1 + 2 * np.log(0.5)) and np.allclose(out[0][1], -1 + np.log(0.5))   # log(coef) per member
    k_max = serve.retrieve(m, [{"1.retrieval": [0.0] * D}] * 3, 1, 200)     # k = V_1
    assert len(k_max) == 3


def test_exclusion_csr_ragged():
    off, ids = exclusion_csr([[5, 5, 1], [], [0, 2]], 3)
    assert off.tolist() == [0, 3, 3, 5] and ids.tolist() == [5, 5, 1, 0, 2] and ids.dtype == np.int32
    off, ids = exclusion_csr([[], []], 2)
    assert off.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        exclusion_csr([[1]], 2)
