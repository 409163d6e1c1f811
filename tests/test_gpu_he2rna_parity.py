"""HE2RNA on its flat parameter buffer computes, bit for bit, what it computed on ``nn.Conv1d`` containers: every forward form, every
gradient, the order in which the autograd path consumes its RNG streams and three fused training steps, against
tests/golden/he2rna_flat_parity.npz -- recorded on the MI355X by tests/golden/make_he2rna_parity.py at the commit in front of the
flat buffer, and recomputed here by the same `record`.  Three stacks of B * N = 60 rows: a fraction of a second each."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_he2rna_parity as mk  # noqa: E402
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.he2rna import He2rnaTrainStep  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(GOLDEN, "he2rna_flat_parity.npz"))


@pytest.mark.parametrize("name", list(mk.STACKS))
def test_every_recorded_array_is_reproduced_bit_for_bit(name):
    _lib.require_gpu()
    want = {k[len(name) + 1:]: _fixture()[k] for k in _fixture().files if k.startswith(name + "/")}
    got = mk.record(name)
    n_tensors = 2 * (len(mk.STACKS[name]["layers"]) + 1)
    assert set(got) == set(want) and len(want) == 8 + 2 * (n_tensors + 1) + 2 * n_tensors
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, k
        assert np.array_equal(got[k], w, equal_nan=True) and np.array_equal(np.isnan(got[k]), np.isnan(w)), k
    # the fixture exercises what it is about: finite predictions, no vanishing gradient tensor, parameters that moved
    assert np.isfinite(want["eval"]).all() and all(np.abs(w).max() > 0 for k, w in want.items() if "grad" in k)
    sd = mk.inputs(name)[0]
    assert all(not np.array_equal(want["fused_final/" + k], v.numpy()) for k, v in sd.items())


@pytest.mark.parametrize("name", list(mk.STACKS))
def test_a_model_moved_to_the_device_trains_to_the_bits_of_one_built_there(name):
    _lib.require_gpu()
    on_device, moved = mk.model(name), mk.model(name, device="cpu")
    assert not moved.flat.is_cuda
    moved.to(mk.DEV)
    moved.device = mk.DEV
    losses = [mk.fused_steps(m, name, 2) for m in (on_device, moved)]
    assert torch.equal(losses[0], losses[1]) and torch.equal(on_device.flat, moved.flat)
    assert not torch.equal(on_device.flat.cpu(), mk.model(name, device="cpu").flat)


def test_a_step_refuses_a_model_that_no_longer_owns_its_buffer():
    """Moved or given another head after the step was built, the model reads another buffer than the one the step's gradient and
    moments describe: the step refuses instead of training a detached copy.  Nothing is launched."""
    _lib.require_gpu()
    _, x, _, y = mk.inputs("layers5x12")
    xb = x.transpose(1, 2).contiguous()
    for change in (lambda m: m.replace_head(mk.G), lambda m: m.to("cpu")):
        m = mk.model("layers5x12")
        tr = He2rnaTrainStep(m, mk.LR)
        change(m)
        with pytest.raises(_lib.SequoiaHipError, match="moved or its head replaced"):
            tr.step(xb, y)
    with pytest.raises(_lib.SequoiaHipError, match="on the GPU"):
        He2rnaTrainStep(mk.model("layers5x12", device="cpu"), mk.LR)
