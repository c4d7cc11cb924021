"""CPU: the host side of the serving compact top -- the two count rules as `serve.py` restates them, checked at their edges,
and the `compact_top=` keyword of the serving calls, which sets rsys_serving_compact_top_set for the length of the call and restores it on
every exit path, an exception included.  No GPU, no library: the model is a stand-in that records the switch."""
import pytest

from recommendersystem_amd import serve


def test_compact_tail_rule_at_its_edges():
    # fits the buffers and at most half of the tokens
    assert serve.compact_top_rows(1, 2, 256)
    assert not serve.compact_top_rows(0, 512, 256)
    assert serve.compact_top_rows(256, 512, 256)
    assert not serve.compact_top_rows(257, 1024, 256)        # one row more than the buffers hold
    assert serve.compact_top_rows(128, 256, 256)
    assert not serve.compact_top_rows(129, 256, 256)         # 2 n_sel = NT + 2
    assert not serve.compact_top_rows(1, 1, 256)


def test_selected_attention_rule_at_its_edges():
    # one selected query per 64-token tile on average: rows * ceil(2 row_len / 64)
    assert serve.compact_top_selected_attention(4, 4, 32)            # 64 tokens: one tile per row
    assert not serve.compact_top_selected_attention(5, 4, 32)
    assert serve.compact_top_selected_attention(8, 4, 33)            # 66 tokens: two tiles per row
    assert not serve.compact_top_selected_attention(9, 4, 33)
    assert serve.compact_top_selected_attention(4 * 32, 4, 1024)     # 2048 tokens: 32 tiles
    assert not serve.compact_top_selected_attention(4 * 32 + 1, 4, 1024)


def test_mode_follows_the_two_rules():
    cap = 256
    assert serve.compact_top_mode(None, 4, 128, cap) == 0                       # rsys_infer without a selection
    assert serve.compact_top_mode(4, 4, 128, cap) == 2                          # one query token per row
    assert serve.compact_top_mode(16, 4, 128, cap) == 2                         # 4 tiles per row
    assert serve.compact_top_mode(17, 4, 128, cap) == 1
    assert serve.compact_top_mode(256, 4, 128, cap) == 1                        # 2 * 256 = 512 <= 1024
    assert serve.compact_top_mode(257, 4, 128, cap) == 0                        # beyond the buffers
    assert serve.compact_top_mode(129, 1, 128, cap) == 0                        # more than half of the 256 tokens
    assert serve.compact_top_mode(2, 4, 128, cap, kind="candidates") == 1       # candidate rows: never the selected-query kernel
    assert serve.compact_top_mode(600, 4, 128, cap, kind="candidates") == 0
    assert serve.compact_top_mode(None, 4, 128, cap, kind="store") == 3


class _Model:
    """records the switch; every forward raises when told to"""

    def __init__(self, on=False, fail=False):
        self.on, self.fail, self.seen = on, fail, []
        self.config = {"max_sequence_length": 8, "vocab_sizes": {"0_matchedid": 10}}
        self.max_rows = 2

    def serving_compact_top(self, on=None):
        if on is not None:
            self.on = bool(on)
        return self.on

    def inference_select(self, d, task, index, **kw):
        self.seen.append(self.on)
        if self.fail:
            raise RuntimeError("forward failed")
        import numpy as np
        return np.zeros((len(index), 4), np.float32) if task == "retrieval" else np.zeros(len(index), np.float32)


def _user():
    ev = {"medium": 0, "matchedid": 1, "history_max_ts": 1.0, "status": 1, "rating": 5.0, "progress": 1.0, "history_status": 0, "history_rating": 0.0}
    return {"user": {"gender": 0, "source": 0, "birthday": 0.0, "created_at": 0.0}, "items": [ev], "timestamp": 2.0, "ranking_items": [2, 3]}


@pytest.mark.parametrize("before", [False, True])
def test_keyword_sets_the_switch_for_the_call_and_restores_it(before):
    m = _Model(on=before)
    serve.predict(m, [_user()], "retrieval", 0, compact_top=True)
    assert m.seen == [True] and m.on is before
    m.seen.clear()
    serve.predict(m, [_user()], "retrieval", 0)
    assert m.seen == [before] and m.on is before


@pytest.mark.parametrize("before", [False, True])
def test_keyword_restores_the_switch_on_an_exception(before):
    m = _Model(on=before, fail=True)
    with pytest.raises(RuntimeError, match="forward failed"):
        serve.predict(m, [_user()], "retrieval", 0, compact_top=True)
    assert m.seen == [True] and m.on is before


def test_every_serving_call_that_runs_a_forward_takes_the_keyword():
    import inspect
    for name in ("predict", "predict_mixed", "predict_ranking_full", "render", "render_users"):
        p = inspect.signature(getattr(serve, name)).parameters
        assert "compact_top" in p and p["compact_top"].default is False, name
