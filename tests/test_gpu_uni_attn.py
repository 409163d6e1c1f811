"""The three attention cores of the UNI embedder on their own -- uni_attn_kernel<float>, uni_attn_mfma_kernel (bf16) and
uni_attn_x3_kernel (split fp16) -- through sq_dbg_uni_attn, which runs the forward pass's own launch (kernel choice, LDS size,
the opt-in to more than 64 KiB).  The bf16 core has no fp32 twin and a whole network at 5e-2 cannot see a leaked padding key
or a wrong query row (tests/test_uni_cases_host.py), so each core is held here to a derived per-element bound against softmax
attention in float64 on exactly the values handed over (tests/uni_attn_cases.py: inputs, bound and its derivation;
tests/test_uni_attn_host.py: the checker accepts a correct kernel's roundings and rejects wrong cores).

2 images x 3 heads, every (image, head) with data of its own; T = each of the 15 token counts the admitted image sizes give and
the tile edges 1, 31, 32, 33, 64, 255, 256; three input families (random, bait, read-back).

Measured on an MI355X (profiles/uni_shape_contract_errors.txt), worst share of the bound over the families and all T: fp32 0.013
(T = 256), f16x3 0.008 (T = 5), bf16 0.624 (T = 2) -- the bf16 core lands on the figures of the CPU emulation of its rounding
points (uni_attn_cases.emulate_bf16_core) to three digits.  No bound had to be widened."""
import pytest
import torch

import uni_attn_cases as ac

pytestmark = pytest.mark.gpu

from sequoia_pub_amd import _lib  # noqa: E402

DTYPE = {"fp32": _lib.SQ_F32, "bf16": _lib.SQ_BF16, "f16x3": _lib.SQ_F16X3}
GUARD = 4096                  # elements behind the output that must stay as they were


def _launch(mode, qkv_dev, o_dev, n, T, H):
    with torch.cuda.device(qkv_dev.device):
        return _lib.lib().sq_dbg_uni_attn(DTYPE[mode], _lib.ptr(qkv_dev), _lib.ptr(o_dev), n, T, H, _lib.stream_ptr(qkv_dev.device))


def run_core(mode, q, k, v):
    """q, k, v float64 [n, H, T, 64] -> (the values handed to the kernel as float64 q, k, v; its output as float64 [n, H, T, 64])."""
    n, H, T, _ = q.shape
    dev = torch.device("cuda:0")
    qkv = ac.pack_qkv(q, k, v).float()
    rows, wide = n * T, H * ac.DH
    if mode == "f16x3":
        hi = qkv.to(torch.float16)
        lo = (qkv - hi.float()).to(torch.float16)
        handed = hi.double() + lo.double()
        src = torch.stack([hi, lo]).to(dev).contiguous()                      # the lo plane rows * 3 wide elements behind the hi plane
        out = torch.full((2 * rows * wide + GUARD,), float("nan"), dtype=torch.float16, device=dev)
    else:
        dt = torch.float32 if mode == "fp32" else torch.bfloat16
        src = qkv.to(dt).to(dev).contiguous()
        handed = src.cpu().double()
        out = torch.full((rows * wide + GUARD,), float("nan"), dtype=dt, device=dev)
    _lib.check(_launch(mode, src, out, n, T, H))
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[-GUARD:]).all()), "the kernel wrote behind its output"
    got = got[:-GUARD].double()
    if mode == "f16x3":
        got = got[:rows * wide] + got[rows * wide:]
    return ac.unpack_qkv(handed, n, H, T), ac.unpack_o(got.reshape(rows, wide), n, H, T)


@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("T", ac.ALL_T)
def test_core_is_inside_its_derived_bound(T, mode):
    """Per element |o - ref| <= kappa A (uni_attn_cases.py), and in the read-back family every row returns its integer."""
    _lib.require_gpu()
    failed = []
    for fam in ac.FAMILIES:
        d = ac.inputs(fam, T)
        (q, k, v), got = run_core(mode, d["q"], d["k"], d["v"])
        if mode != "f16x3":
            assert torch.equal(q, d["q"]) and torch.equal(k, d["k"]) and torch.equal(v, d["v"])      # bf16-exact: nothing rounded on the way
        ok, ratio = ac.verdict(mode, got, q, k, v, d.get("perm"))
        print(f"uni attention {mode:5s} T {T:3d} {fam:8s}: {ratio:.3f} of the bound")
        if not ok:
            failed.append((fam, ratio))
    assert not failed, failed


@pytest.mark.parametrize("mode", ac.MODES)
def test_hook_refuses_what_it_cannot_run_and_runs_afterwards(mode):
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16x3": torch.float16}[mode]
    planes = 2 if mode == "f16x3" else 1
    buf = torch.zeros(planes * 2 * 257 * 3 * 3 * 64 + 64, dtype=dt, device=dev)
    out = torch.zeros(planes * 2 * 257 * 3 * 64 + 64, dtype=dt, device=dev)
    for T in (0, 257):
        with pytest.raises(_lib.SequoiaHipError, match=f"n_tokens={T}"):
            _lib.check(_launch(mode, buf, out, 2, T, 3))
    with pytest.raises(_lib.SequoiaHipError, match="16-byte aligned"):
        _lib.check(_launch(mode, buf[1:], out, 2, 5, 3))
    with pytest.raises(_lib.SequoiaHipError, match="16-byte aligned"):
        _lib.check(_launch(mode, buf, out[1:], 2, 5, 3))
    with pytest.raises(_lib.SequoiaHipError, match="dtype"):
        _lib.check(_lib.lib().sq_dbg_uni_attn(_lib.SQ_BF16X3, _lib.ptr(buf), _lib.ptr(out), 2, 5, 3, _lib.stream_ptr(dev)))
    d = ac.inputs("random", 37)
    (q, k, v), got = run_core(mode, d["q"], d["k"], d["v"])
    assert ac.verdict(mode, got, q, k, v)[0]
