"""What the item-similarity model (similarity.py) and the search model (search.py) share: each is a device handle of its own with one
trainable matrix and a scalar `logit_scale` (csrc/encoder_handle.hpp), reached through C entry points that differ in their prefix only,
and both training loops stop early and write checkpoints the same way."""
import ctypes as C
import os

import numpy as np

from ._lib import check, lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class EncoderHandle:
    """The calls of an rsys_sim / rsys_search handle `self.h` that differ in the prefix only.  A subclass sets _PREFIX and has
    `_tensor(name)`: the shape of a trainable parameter."""

    _PREFIX = None

    def _fn(self, name):
        return getattr(lib(), f"{self._PREFIX}_{name}")

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def param_get(self, name, grad=False):
        out = np.zeros(self._tensor(name), np.float32)
        check(self._fn("grad_get" if grad else "param_get")(self.h, name.encode(), _ptr(out), out.size))
        return out

    def param_set(self, name, value):
        v = np.ascontiguousarray(np.asarray(value, np.float32).reshape(self._tensor(name)))
        check(self._fn("param_set")(self.h, name.encode(), _ptr(v), v.size))

    def get_temperature(self):
        """the raw parameter, not its exponential"""
        return float(self.param_get("logit_scale"))

    def zero_grad(self):
        check(self._fn("zero_grad")(self.h))

    def adamw_step(self, lr, clip=1.0):
        """clip_grad_norm_ + GradScaler.step(AdamW) + zero_grad; returns (norm, skipped)"""
        norm, skipped = C.c_float(0), C.c_int32(0)
        check(self._fn("adamw_step")(self.h, lr, clip, C.byref(norm), C.byref(skipped)))
        return norm.value, bool(skipped.value)

    def adamw_state(self, name):
        m, v = np.zeros(self._tensor(name), np.float32), np.zeros(self._tensor(name), np.float32)
        step = C.c_int32(0)
        check(self._fn("adamw_state_get")(self.h, name.encode(), _ptr(m), _ptr(v), m.size, C.byref(step)))
        return m, v, step.value


class EarlyStopper:
    """stops if the score does not decrease by rtol in `patience` epochs (pairwise_ltr.py:290-315, search/train.py:208-232)"""

    def __init__(self, patience, rtol):
        self.patience = patience
        self.rtol = rtol
        self.counter = 0
        self.stop_score = float("inf")
        self.stop = False
        self.saved_score = float("inf")
        self.save_model = False

    def __call__(self, score):
        assert not self.stop
        if score < self.stop_score * (1 - self.rtol):
            self.counter = 0
            self.stop_score = score
        else:
            self.counter += 1
            if self.counter >= self.patience:
                self.stop = True
        if score < self.saved_score:
            self.saved_score = score
            self.save_model = True
        else:
            self.save_model = False


def write_checkpoint(stem, model, epoch, training_loss, test_loss, save, datadir, medium):
    """{stem}.{m}.npz under the reference's state-dict names (+ epoch and losses) when `save`, and a row of {stem}.{m}.csv (header
    written at epoch -1)"""
    if save:
        d = dict(model.state_dict())
        d.update(epoch=np.array(epoch), training_loss=np.array(training_loss), test_loss=np.array(test_loss))
        np.savez(os.path.join(datadir, f"{stem}.{medium}.npz"), **d)
    csv_fn = os.path.join(datadir, f"{stem}.{medium}.csv")
    if epoch < 0:
        with open(csv_fn, "w") as f:
            f.write(",".join(["epoch", "training_loss", "test_loss", "saved"]) + "\n")
    with open(csv_fn, "a") as f:
        f.write(",".join(str(x) for x in [epoch, training_loss, test_loss, 1 if save else 0]) + "\n")


def load_checkpoint(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}
