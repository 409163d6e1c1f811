"""The per-block ResNet-50 reference of tests/resnet_tap_cases.py, the host side (no GPU):
  a. its pieces, chained in float64 without rounding, are the oracle's forward_extract;
  b. its own error -- the emulation evaluated on the CPU in float32 against float64 -- sits under the bounds of the case table
     with the stated margin at every row (the figures are printed);
  c. localised indexing mistakes injected into the float32 evaluation break the criterion at the tap of their block while
     the 2048 features move by less than the 5e-2 the bf16 golden test allows: what the tap tests see and the feature tests cannot."""
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import resnet_tap_cases as tc
from gpu_util import rel_err
from oracle import resnet_oracle as ro

BF16_GOLDEN_TOL = 5e-2            # tests/test_gpu_resnet.py: the bf16 features against the golden


@pytest.mark.parametrize("row_id", ["224x224-n1", "208x265-n2"])
def test_pieces_chained_in_float64_are_the_oracle(row_id):
    sd = OrderedDict((k, v.double()) for k, v in tc.state_dict("std").items())
    x = tc.normalised(row_id).double()
    emu = tc.Emu(None, tc.operands_from_state_dict(sd))
    with tc.oracle_threads(), torch.no_grad():
        feats, inter = ro.forward_extract(sd, x, return_intermediates=True)
        conv1 = emu.stem(x, parts=True)[1]
        taps = emu.chain(x)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    assert [tuple(t.shape) for t in taps] == tc.tap_shapes(*x.shape[:1], *x.shape[2:])
    errs = dict(conv1=rel_err(nchw(conv1), inter["conv1"]), maxpool=rel_err(nchw(taps[0]), inter["maxpool"]),
                features=rel_err(tc.Emu.features(taps[-1]), feats))
    last = 0
    for li, nb in enumerate(ro.LAYERS):
        last += 2 * nb
        errs[f"layer{li + 1}"] = rel_err(nchw(taps[last]), inter[f"layer{li + 1}"])
    print(row_id, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-12, errs


def test_decoded_operands_are_the_packed_state_dict():
    """`decode` reads the entry's buffers by the header's layout: in every mode it must give back the float64 fold of the state
    dict to the precision of that mode's weight format (half an ulp: fp32 2^-24, bf16 2^-8; two planes: fp16 2^-22, bf16 2^-16 -- of the
    row's largest weight), and the K-tile-major order must be undone (a wrong order is an error of order one)."""
    exact = tc.operands_from_state_dict(OrderedDict((k, v.double()) for k, v in tc.state_dict("std").items()))
    bound = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16x3": 2.0 ** -22, "bf16x3": 2.0 ** -16}
    for mode in tc.MODES:
        ops = tc.operands(mode, "std")
        assert ops.desc == exact.desc
        for i in range(len(exact.w)):
            w = ops.w[i] * ops.cs[i].view(-1, 1, 1, 1)
            rowmax = exact.w[i].abs().amax(dim=(1, 2, 3), keepdim=True)
            assert float(((w - exact.w[i]).abs() / rowmax).max()) <= bound[mode], (mode, i)
            assert float((ops.b[i] - exact.b[i]).abs().max()) <= 2.0 ** -24 * float(exact.b[i].abs().max()), (mode, i)


FLOOR_CASES = [(m, r["id"], "std") for m in tc.MODES for r in tc.ROWS] + [(m, tc.WIDE_ROW, "wide") for m in ("f16x3", "bf16x3")]


@pytest.mark.parametrize("mode,row_id,weights", FLOOR_CASES)
def test_floor_of_the_reference_leaves_the_margin(mode, row_id, weights):
    taps = tc.host_chain(row_id, mode, weights)
    ref = tc.teacher_forced(tc.Emu(mode, tc.operands(mode, weights)), taps, tc.normalised(row_id))
    worst = {}
    for i in range(tc.N_TAPS):
        m = tc.measure(taps[i], ref[i])
        k = tc.tap_kind(i)
        if k not in worst or m["ratio"] > worst[k]["ratio"]:
            worst[k] = dict(m, tap=i)
        worst["unequal"] = max(worst.get("unequal", 0.0), m["unequal"])
    f32 = tc.Emu.features(taps[-1])
    ferr = rel_err(f32, tc.Emu.features(taps[-1].double()))
    print(f"\nfloor {mode} {row_id} {weights}: " + ", ".join(f"{k} {worst[k]['ratio']:.3e} (tap {worst[k]['tap']} {tc.tap_name(worst[k]['tap'])})"
                                                          for k in ("stem", "t1", "y")) +
          f"; unequal share {worst['unequal']:.4%}; features {ferr:.2e}; r = {tc.bound(mode, weights)}")
    for k in ("stem", "t1", "y"):
        if mode == "bf16":
            assert worst[k]["ratio"] <= tc.BF16_R, tc.where(f"{k}: tap {worst[k]['tap']}", worst[k])
        else:
            assert tc.MARGIN * worst[k]["ratio"] <= tc.bound(mode, weights)[k], tc.where(f"{k}: tap {worst[k]['tap']}", worst[k])
    if mode == "bf16":
        assert worst["unequal"] <= tc.BF16_UNEQUAL_CAP / 4
    assert tc.MARGIN * ferr <= tc.FEATURE_TOL
    assert not tc.violations(mode, taps, ref, weights=weights)


# ---- injected mistakes ----------------------------------------------------------------------------------------------------

def _wrap(x):
    """The 3x3's right-hand zero padding replaced by the next row's first pixel (a flat-row wrap)."""
    p = F.pad(x, (0, 0, 1, 1, 1, 1))
    H = x.shape[1]
    p[:, 1:H, -1] = x[:, 1:, 0]
    return p


def _ragged(emu, i, t1, t2):
    """The last output row of the batch's last image computed from a zero input row (a ragged tile tail)."""
    z = t1.clone()
    z[-1, -1] = 0
    t2 = t2.clone()
    t2[-1, -1] = emu.q(emu.conv(i, z, True))[-1, -1]
    return t2


def _missing_tap(emu, i, a, acc):
    """The bottom-right output pixel of the 3x3 misses its (kh, kw) = (1, 0) tap."""
    s = emu.ops.desc[i][3]
    ih, iw = (acc.shape[1] - 1) * s, (acc.shape[2] - 1) * s - 1
    acc = acc.clone()
    acc[:, -1, -1] -= a[:, ih, iw] @ emu.ops.w[i][:, :, 1, 0].to(a.dtype).t()
    return acc


def _pool_ignores_last_column(c):
    """The last max-pool column ignores the last conv1 column (post-ReLU values: 0 never wins against a column that counts)."""
    c = c.clone()
    c[:, :, -1] = 0
    return c


def _conv1_misses_tap_column(emu, i, a, acc):
    """The last conv1 column misses its right-most in-image tap column."""
    W, ow = a.shape[2], acc.shape[2] - 1
    kw = min(6, W - 1 - (2 * ow - 3))
    wz = torch.zeros_like(emu.ops.w[0])
    wz[:, :, :, kw] = emu.ops.w[0][:, :, :, kw]
    part = F.conv2d(a.permute(0, 3, 1, 2), wz.to(a.dtype), stride=2, padding=3).permute(0, 2, 3, 1)
    acc = acc.clone()
    acc[:, :, -1] -= part[:, :, -1]
    return acc


def _block(li, b):
    return tc.BLOCKS.index((li - 1, b))


def _mistakes():
    out = []
    for li, b in ((1, 1), (2, 2), (3, 3), (4, 1)):
        out.append((f"wrap-layer{li}.{b}", _block(li, b), lambda ci: {(ci + 1, "input"): _wrap}))
    for li, b in ((1, 2), (2, 1), (3, 0)):
        out.append((f"ragged-layer{li}.{b}", _block(li, b), lambda ci: {(ci + 1, "out"): _ragged}))
    for li, b in ((1, 0), (2, 0), (3, 2)):
        out.append((f"tap-layer{li}.{b}", _block(li, b), lambda ci: {(ci + 1, "acc"): _missing_tap}))
    out.append(("pool-last-column", None, lambda ci: {(0, "map"): _pool_ignores_last_column}))
    out.append(("conv1-tap-column", None, lambda ci: {(0, "acc"): _conv1_misses_tap_column}))
    return out


MISTAKES = _mistakes()
MISTAKE_ROW = "224x224-n1"


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", [m[0] for m in MISTAKES])
def test_injected_mistake_breaks_its_tap_and_hides_in_the_features(name, mode):
    _, k, hooks = next(m for m in MISTAKES if m[0] == name)
    ops = tc.operands(mode, "std")
    x = tc.normalised(MISTAKE_ROW)
    base = tc.host_chain(MISTAKE_ROW, mode, "std")
    bad_emu = tc.Emu(mode, ops, prec=torch.float32, mutate=hooks(tc.conv_index(k) if k is not None else 0))
    with tc.oracle_threads(), torch.no_grad():
        taps = bad_emu.chain(x, start=None if k is None else (k, base))
    tap = 0 if k is None else 2 * k + 2
    ref = tc.teacher_forced(tc.Emu(mode, ops), taps, x, which=[tap])
    m = tc.measure(taps[tap], ref[tap])
    moved = rel_err(tc.Emu.features(taps[-1]), tc.Emu.features(base[-1]))
    print(f"\nmistake {name} {mode}: tap {tap} {tc.tap_name(tap)} ratio {m['ratio']:.3e} (r {tc.bound(mode, 'std')[tc.tap_kind(tap)]:.3e}), "
          f"unequal {m['unequal']:.3%}, at {m['index']}; features moved {moved:.3e}")
    assert tc.violations(mode, taps, ref), "the criterion does not see this mistake"
    assert not tc.violations(mode, base, tc.teacher_forced(tc.Emu(mode, ops), base, x, which=[tap]))
    assert 0 < moved < BF16_GOLDEN_TOL
