"""Every ResNet-50 block alone against float64 (tests/resnet_tap_cases.py has the reference, the rows and the bounds):
sq_dbg_resnet50_taps runs the forward of sq_resnet50_extract_hw and copies out the stem's output and every bottleneck's t1
and y; each tap is checked against float64 arithmetic on the HIP path's own earlier taps, in all four numeric modes, on the
default route, on every route switch (bit-equal taps), with the LDS-resident 3x3 on and off, and in both input forms.

Measured on an MI355X, worst |got - ref| / (|ref| + rms) over the three rows, stem / t1 / y (the bounds r in brackets; every
case prints its figures before it asserts, profiles/resnet_tap_errors.txt keeps them):
  fp32    9.7e-07 / 5.4e-06 / 6.5e-06   (3.76e-06 / 1.24e-05 / 2.04e-05)
  f16x3   6.7e-07 / 3.3e-06 / 5.6e-06   (3.92e-06 / 1.24e-05 / 1.88e-05);  wide-range weights 7.3e-07 / 9.8e-06 / 9.4e-06 (3.48e-06 / 2.76e-05 / 3.88e-05)
  bf16x3  1.1e-05 / 2.4e-05 / 4.6e-05   (4.8e-05 / 1.0e-04 / 1.96e-04);    wide-range weights 1.3e-05 / 6.8e-05 / 8.9e-05 (5.2e-05 / 2.76e-04 / 3.52e-04)
  bf16    3.8e-03 / 5.4e-03 / 6.9e-03   (2^-7 = 7.8e-03), at most 0.17 % of a tap's elements off the rounded reference (0.26 % with the
          LDS-resident 3x3 from one tile on; the cap is 1 %).
No bound had to be widened and no kernel fault was found: all routes give bit-equal taps."""
import os
import subprocess
import sys

import pytest
import torch

import resnet_tap_cases as tc
from sequoia_pub_amd import _lib

pytestmark = pytest.mark.gpu

ROUTE_SWITCHES = ("SQ_RESNET_NO_FUSE", "SQ_RESNET_NO_CHAIN", "SQ_RESNET_NO_CHAIN_DS", "SQ_RESNET_NO_TAIL", "SQ_RESNET_NO_CHAINW",
                  "SQ_RESNET_NO_DUAL", "SQ_RESNET_NO_STEM_REDUCE")
ROUTE_ROW = "193x193-n3"          # every map odd, three images: the fused tails, chains and the stem reduce all apply
HALO_ROW = "193x193-n3"           # 25 x 25, 13 x 13, 7 x 7 maps: image boundaries and a ragged end inside the staged tiles
FORM_ROW = "208x265-n2"
AFTER_REFUSAL = "224x224-n1"


def _report(what, mode, weights, row_id, taps):
    """The figures of one forward: worst ratio per kind of tap and the largest unequal share (printed before anything is asserted)."""
    ref = tc.teacher_forced(tc.Emu(mode, tc.operands(mode, weights)), taps, None, which=range(1, tc.N_TAPS))
    ref[0] = tc.stem_reference(row_id, mode, weights)
    worst, unequal = {}, (0.0, 0)
    for i in sorted(ref):
        m = tc.measure(taps[i], ref[i])
        k = tc.tap_kind(i)
        if k not in worst or m["ratio"] > worst[k][0]:
            worst[k] = (m["ratio"], i)
        unequal = max(unequal, (m["unequal"], i))
    print(f"\n{what} {mode} {weights}: " + ", ".join(f"{k} {v[0]:.3e} (tap {v[1]} {tc.tap_name(v[1])})" for k, v in worst.items()) +
          f"; unequal share at most {unequal[0]:.4%} (tap {unequal[1]}); r = {tc.bound(mode, weights)}")
    return ref


def _check(what, mode, weights, row_id, taps, feats):
    ref = _report(what, mode, weights, row_id, taps)
    bad = tc.check_forward(mode, weights, row_id, taps, feats, ref)
    assert not bad, f"{what} {mode} {weights}: {len(bad)} violations\n" + "\n".join(bad[:8])


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("row_id", [r["id"] for r in tc.ROWS])
def test_taps_default_route(row_id, mode):
    _lib.require_gpu()
    taps, feats = tc.run_taps(mode, "std", row_id)
    _check(row_id, mode, "std", row_id, taps, feats)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_taps_wide_range_weights(mode):
    """Weight rows over two decades, folded BN scales over four: the per-channel factors of the fp16 planes at work."""
    _lib.require_gpu()
    taps, feats = tc.run_taps(mode, "wide", tc.WIDE_ROW)
    _check(tc.WIDE_ROW, mode, "wide", tc.WIDE_ROW, taps, feats)


@pytest.mark.parametrize("mode", tc.MODES)
def test_taps_normalised_fp32_input(mode):
    """The other input form: normalised fp32 NCHW, the tensor the reference feeds forward_extract."""
    _lib.require_gpu()
    taps, feats = tc.run_taps(mode, "std", FORM_ROW, form="f32")
    _check(FORM_ROW + " f32 nchw", mode, "std", FORM_ROW, taps, feats)


@pytest.mark.parametrize("mode", tc.MODES)
def test_route_switches_give_bit_equal_taps(mode, monkeypatch):
    """Every switch the forward reads per call: the same bits in all 33 taps and the features as the default route."""
    _lib.require_gpu()
    for s in ROUTE_SWITCHES:
        monkeypatch.delenv(s, raising=False)
    base, base_f = tc.run_taps(mode, "std", ROUTE_ROW)
    for s in ROUTE_SWITCHES:
        monkeypatch.setenv(s, "1")
        taps, feats = tc.run_taps(mode, "std", ROUTE_ROW)
        monkeypatch.delenv(s)
        differ = [f"{i} {tc.tap_name(i)} ({int((a != b).sum())} of {a.numel()})" for i, (a, b) in enumerate(zip(taps, base)) if not torch.equal(a, b)]
        assert not differ, f"{mode} {s}=1: taps differ from the default route: {differ[:6]}"
        assert torch.equal(feats, base_f), f"{mode} {s}=1: features differ"


@pytest.mark.parametrize("halo", ["1", "0"])
@pytest.mark.parametrize("mode", ["bf16", "f16x3"])
def test_halo_staged_3x3_taps(mode, halo, tmp_path):
    """conv_halo.hip / conv_halo_x3.hip (input tile resident in LDS) on and off, from the smallest tile count on: both must meet
    the criterion against the reference (their K order differs, so they need not agree bit for bit)."""
    _lib.require_gpu()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "taps.pt")
    env = dict(os.environ, SQ_CONV_HALO=halo, SQ_CONV_HALO_MIN_TILES="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "resnet_taps_worker.py"), mode, HALO_ROW, out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = torch.load(out)
    row = tc.BY_ID[HALO_ROW]
    taps = tc.as_taps(z["taps"], tc.tap_offsets(row["n"], row["H"], row["W"]), row["n"], row["H"], row["W"])
    _check(f"{HALO_ROW} SQ_CONV_HALO={halo}", mode, "std", HALO_ROW, taps, z["feats"])


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_refusals_name_the_reason_and_leave_the_process_usable(mode):
    _lib.require_gpu()
    with pytest.raises(_lib.SequoiaHipArgError, match="taps buffer of"):
        tc.run_taps(mode, "std", AFTER_REFUSAL, short_by=1)
    with pytest.raises(_lib.SequoiaHipArgError, match=r"192 x 224.*\[193, 416\]"):
        tc.run_taps(mode, "std", AFTER_REFUSAL, shape=(192, 224))
    with pytest.raises(_lib.SequoiaHipArgError, match=r"224 x 417.*\[193, 416\]"):
        tc.run_taps(mode, "std", AFTER_REFUSAL, shape=(224, 417))
    assert tc.tap_offsets(2, 208, 265)[33] == sum(int(torch.Size(s).numel()) for s in tc.tap_shapes(2, 208, 265))
    taps, feats = tc.run_taps(mode, "std", AFTER_REFUSAL)
    _check(AFTER_REFUSAL + " after the refusals", mode, "std", AFTER_REFUSAL, taps, feats)
