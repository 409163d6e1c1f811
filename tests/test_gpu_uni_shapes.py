"""The UNI embedder across the shapes check_cfg admits (tests/uni_cases.py), in its three modes, against the float64 oracle.
tests/test_uni_cases_host.py shows on the CPU that every row is a fair test: the float32 oracle a decade inside the fp32
bound, the bfloat16 oracle inside the bf16 bound, and a wrong attention core outside the fp32 / f16x3 bound.

Per row and mode: extract_patches_u8 within the mode's tolerance (max-norm and per element), the normalised-tensor call form
m(x) next to it, a batch equal to its single-patch calls bit for bit, sub_batch < n the same bits, and in f16x3 no overflow
re-run.  Refused configurations fail by message, and a valid row matches afterwards in the same process."""
import warnings

import numpy as np
import pytest
import torch

import uni_cases as uc
from gpu_util import assert_allclose_rel, rel_err

pytestmark = pytest.mark.gpu

from oracle import uni_oracle  # noqa: E402  (checker only)
from sequoia_pub_amd import _abi, _lib  # noqa: E402
from sequoia_pub_amd.uni import UniViT  # noqa: E402


def _net(case, mode):
    m = UniViT(compute_dtype=mode, **uc.model_kwargs(case))
    m.load_state_dict(uc.state_dict(case))
    return m.to("cuda:0").eval()


def _check_row(c, mode):
    ref = uc.reference(c)
    p = uc.patches(c)
    m = _net(c, mode)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # an overflow re-run warns: none may happen
        got_t = m.extract_patches_u8(p)
        direct = m(uni_oracle.transform_patch_u8(p)).cpu().numpy()
        singles = torch.cat([m.extract_patches_u8(p[i:i + 1]) for i in range(c["n"])], 0)
        split = m.extract_patches_u8(p, sub_batch=max(1, c["n"] - 1))
    got = got_t.cpu().numpy()
    e = rel_err(got, ref)
    d_ref = rel_err(uc.reference(c, torch.float32), ref)
    print(f"{c['id']} {mode}: {e:.3e} off the float64 oracle (float32 oracle: d_ref {d_ref:.2e}); m(x) vs u8 {rel_err(direct, got):.2e}   [{c['branch']}]")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert e < uc.TOL[mode]
    assert_allclose_rel(got, ref, uc.TOL[mode], f"{c['id']} {mode}")
    assert rel_err(direct, got) < uc.TOL_DIRECT[mode]
    assert torch.equal(singles, got_t), "a batch differs from its single-patch calls"
    assert torch.equal(split, got_t), "sub_batch < n changed the bits"
    if mode == "f16x3":
        assert getattr(m, "last_nonfinite_reruns", 0) == 0


@pytest.mark.parametrize("mode", uc.MODES)
@pytest.mark.parametrize("cid", [c["id"] for c in uc.CASES])
def test_row_matches_the_float64_oracle(cid, mode):
    _lib.require_gpu()
    _check_row(uc.BY_ID[cid], mode)


@pytest.mark.parametrize("mode", uc.MODES)
def test_refused_shapes_fail_by_message_and_leave_the_process_usable(mode):
    _lib.require_gpu()
    for r in uc.refusals(_abi.CONSTANTS["SQ_UNI_MAX_DEPTH"]):
        with pytest.raises(_lib.SequoiaHipError, match=r["match"]):
            UniViT(compute_dtype=mode, **uc.model_kwargs(r))
    c = uc.BY_ID[uc.AFTER_REFUSAL]
    m = _net(c, mode)
    for S in (c["img"] - 16, c["img"] + 16):                  # patches of another size than the position embedding's
        with pytest.raises(ValueError, match=f"patches are {S} x {S}"):
            m.extract_patches_u8(np.zeros((2, S, S, 3), dtype=np.uint8))
        with pytest.raises(ValueError, match=f"patches are {S} x {S}"):
            m(torch.zeros(2, 3, S, S))
    _check_row(c, mode)
