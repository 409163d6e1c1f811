"""Case table and per-block reference of the ResNet-50 tap tests, shared by tests/test_resnet_taps_host.py (CPU: is the
reference's own error inside the bounds, and do the bounds see localised mistakes?) and tests/test_gpu_resnet_taps.py (GPU:
every tensor sq_dbg_resnet50_taps copies out against float64 arithmetic).

The reference is teacher-forced: tap k is checked against float64 arithmetic on the HIP path's OWN earlier taps, so an
error shows at full size in the block that makes it and nowhere else.

    stem   = Q(maxpool3x3s2(relu(conv7x7s2(Qin(input)) * cs + b)))            from the input patches
    t1_k   = Q(relu(conv1(x_k) * cs + b))                                     x_k = the stem tap (k = 0) or the y tap of block k - 1
    y_k    = Q(relu((conv3(t2) * cs + b) + idn)),  t2 = Q(relu(conv2(t1_k) * cs + b)),  idn = x_k or Q(ds(x_k) * cs + b)
    feats  = sum of the top-left 7 x 7 of the last y tap / 49

The operands are what the kernels read, decoded from the very buffers handed to the entry by the layout
include/sequoia_hip.h states (`decode`): packed BN-folded weights [cout][kh][kw][cin] and biases; in bf16 the bf16 weights;
in the split modes hi + lo out of the K-tile-major planes (conv 0: [64][152] rows) with the per-channel factors cs that the
bias array carries behind the biases (cs = 1 / s; cs = 1 outside the split modes).  BN folding is not re-derived here.

Rounding points Q (where each mode STORES; the accumulators are fp32 throughout):
  fp32    nowhere.  csrc/gemm_epi.h epi_apply: acc + bias (+ residual), ReLU, fp32 store.
  bf16    the stem's input after the fp32 normalisation (csrc/conv1.hip: the look-up table / the staged window is bf16), and
          every stored activation: epi_apply's st8h (pack_bf16x2, round to nearest even) behind bias + residual + ReLU --
          t1, t2, the downsample output (stored without activation, read back as the bf16 residual) and y.  The fused
          tail / chain kernels keep t2 on the CU but round it to bf16 as the MFMA operand; the bit-identity tests
          (tests/test_gpu_resnet.py) tie them to the unfused route, so one emulation serves both.
  f16x3 / bf16x3   v -> hi + lo, hi = cvt(v), lo = cvt(v - hi) (csrc/x3_fmt.h x3_split8) at the same places: the stem's
          normalised input (csrc/conv1_x3.hip), t1, t2, y, and the downsample output -- also where it rides in the expand
          launch as a second product (csrc/gemm_x3.hip: d = sd * accd + bd is packed to hi / lo and joined before the add).
          Epilogue: (cs * acc + b) + idn, x3_relu, split.  A product is a_hi w_hi + a_hi w_lo + a_lo w_hi; the float64
          reference multiplies the joined operands (the a_lo w_lo term it includes is part of the measured floor).
  The max-pool commutes with Q (both roundings are monotonic), the 7 x 7 mean is fp32 on the joined values.

Criterion, per tap and element, rms = the RMS of the reference tap:  |got - ref| <= r * (|ref| + rms).
  bf16: r = 2^-7 (one bf16 ulp of a reference rounded to bf16: the format), and at most BF16_UNEQUAL_CAP of a tap's elements
        may differ AT ALL from the rounded reference.
  fp32, f16x3, bf16x3: r = 4 x the reference's own floor -- this module's emulation evaluated on the CPU in float32 (split
        modes: the three float32 products) against float64, the worst over the table's rows; the factor 4 because the MFMAs
        sum K in another order than the CPU does.  FLOOR holds the measured figures, R the bounds, per weight set;
        tests/test_resnet_taps_host.py measures the floors again and asserts the margin.  A row whose floor does not leave
        that margin is replaced by another shape reaching the same edge, never given a looser bound.
  features: 1e-6 in the rel_err form (a sum of 49 fp32 terms) against the mean of the last y TAP.

References that do not depend on the HIP taps (operands, inputs, the stem, the CPU float32 chain of the host test) are
cached per row, weight set, input form and emulation; the block references are functions of the taps handed in."""
import contextlib
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import resnet_oracle as ro
from sequoia_pub_amd import _lib, resnet as rn, synth

MODES = ("fp32", "bf16", "f16x3", "bf16x3")
N_TAPS = 33
BLOCKS = [(li, b) for li, nb in enumerate(ro.LAYERS) for b in range(nb)]          # 16 bottlenecks: (layer index 0..3, block)

# patch height, width, patches: the smallest shapes that still reach the edges; seed: the synth.patches_u8 slide the patches are
# cropped from.  The 193 x 193 row was first drawn from slide 31: in bf16 mode ONE element of layer4.0.y (of 301 056) then sits at
# 8.2e-3 > 2^-7 already in the CPU float32 evaluation (next worst 3.4e-3) -- the bf16 rounding of the downsample output flips
# under an output where expand and identity nearly cancel, an ulp of the large summand against the bound of the small sum.
# That floor does not leave the bound, so by the rule above the row's input was replaced (slide 41: 6.9e-3); the shape stayed.
ROWS = [
    dict(id="193x193-n3", H=193, W=193, n=3, seed=41,
         why="the admitted minimum: conv1 map 97 x 97, then 49, 25, 13, 7 -- every map odd, pixel totals no multiple of the 128-pixel tile"),
    dict(id="224x224-n1", H=224, W=224, n=1, seed=32,
         why="the square entry's rule: 112, 56, 28, 14, 7; 24.5 tiles of 128 pixels per image"),
    dict(id="208x265-n2", H=208, W=265, n=2, seed=33,
         why="even and odd maps mixed: 104 x 133, 52 x 67, 26 x 34, 13 x 17, 7 x 9 -- final-map columns the pool never reads"),
]
BY_ID = {r["id"]: r for r in ROWS}
WIDE_ROW = "224x224-n1"            # the wide-range weight set (split modes) runs at this row

BF16_R = 2.0 ** -7
BF16_UNEQUAL_CAP = 0.01
FEATURE_TOL = 1e-6
MARGIN = 4.0
# The reference's own floor per (mode, weight set) and kind of tap: the worst over ROWS (wide set: WIDE_ROW) of
# max |float32 emulation - float64 reference| / (|ref| + rms), as tests/test_resnet_taps_host.py measures and prints it,
# rounded up to two digits.  r = MARGIN x floor.
FLOOR = {
    ("fp32", "std"): dict(stem=9.4e-7, t1=3.1e-6, y=5.1e-6),         # 9.344e-07, 3.027e-06, 5.073e-06: all three at 193 x 193
    ("f16x3", "std"): dict(stem=9.8e-7, t1=3.1e-6, y=4.7e-6),        # 9.747e-07 (224), 3.054e-06 (208 x 265), 4.697e-06 (193)
    ("bf16x3", "std"): dict(stem=1.2e-5, t1=2.5e-5, y=4.9e-5),       # 1.125e-05, 2.411e-05, 4.896e-05: all three at 193 x 193
    ("f16x3", "wide"): dict(stem=8.7e-7, t1=6.9e-6, y=9.7e-6),       # 8.656e-07, 6.831e-06, 9.606e-06
    ("bf16x3", "wide"): dict(stem=1.3e-5, t1=6.9e-5, y=8.8e-5),      # 1.256e-05, 6.802e-05, 8.711e-05
}
R = {key: {k: MARGIN * v for k, v in f.items()} for key, f in FLOOR.items()}
R[("bf16", "std")] = dict(stem=BF16_R, t1=BF16_R, y=BF16_R)


def bound(mode, weights="std"):
    return R[(mode, weights)]


ORACLE_THREADS = 16


@contextlib.contextmanager
def oracle_threads():
    """The CPU arithmetic runs on 16 threads whatever the machine's core count (never sized from os.cpu_count())."""
    n = torch.get_num_threads()
    torch.set_num_threads(ORACLE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def tap_kind(i):
    return "stem" if i == 0 else ("t1" if i % 2 else "y")


def tap_name(i):
    if i == 0:
        return "stem"
    li, b = BLOCKS[(i - 1) // 2]
    return f"layer{li + 1}.{b}.{'t1' if i % 2 else 'y'}"


def tap_shapes(n, H, W):
    """NHWC shapes of the 33 taps, in the order include/sequoia_hip.h states."""
    h, w = -(-(-(-H // 2)) // 2), -(-(-(-W // 2)) // 2)
    out = [(n, h, w, 64)]
    for li, b in BLOCKS:
        out.append((n, h, w, ro.PLANES[li]))
        if b == 0 and li > 0:
            h, w = -(-h // 2), -(-w // 2)
        out.append((n, h, w, 4 * ro.PLANES[li]))
    return out


# ---- inputs and operands ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def patches(row_id):
    r = BY_ID[row_id]
    p = synth.patches_u8(r["seed"], n_patches=r["n"], size=max(r["H"], r["W"]))
    return np.ascontiguousarray(p[:, :r["H"], :r["W"]])


def normalised(row_id):
    """fp32 NCHW, the reference's fp32 transform of the uint8 patches (what the fused normalisation reproduces bit for bit)."""
    return ro.transform_patch_u8(torch.from_numpy(patches(row_id))).contiguous()


@functools.lru_cache(maxsize=None)
def state_dict(weights):
    if weights == "std":
        return ro.init_resnet50_state_dict(seed=99, perturb_bn=True)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet50_wide_bn.npz")
    return ro.init_resnet50_state_dict_wide(123, running_stats=np.load(golden))


@functools.lru_cache(maxsize=None)
def packed(mode, weights):
    """(weights, bias) CPU tensors exactly as sequoia_pub_amd.resnet hands them to the entry in `mode`."""
    w, b = rn.pack_weights(state_dict(weights))
    dt = _lib.DTYPES[mode]
    if dt in (_lib.SQ_BF16X3, _lib.SQ_F16X3):
        w, b = rn.split_planes(w, b, dt)
    elif dt == _lib.SQ_BF16:
        w = w.to(torch.bfloat16)
    return w.contiguous(), b.contiguous()


class Operands:
    """Per convolution i (sq_resnet50_layout order): w[i] float64 [cout, cin, k, k] (split modes: hi + lo; whi / wlo the
    planes), b[i], cs[i] float64 [cout]; desc[i] = (cin, cout, k, stride, pad)."""

    def __init__(self):
        self.w, self.whi, self.wlo, self.b, self.cs, self.desc = [], [], [], [], [], []


def decode(mode, w, b):
    """The operands out of the buffers passed to the entry, by the layout the header states."""
    lay = rn.resnet50_layout()
    split = mode in ("f16x3", "bf16x3")
    ops = Operands()
    if split:
        planes = w.view(torch.float16 if mode == "f16x3" else torch.bfloat16)
        assert planes.numel() == 2 * lay.w_total and b.numel() == 2 * lay.b_total
        planes = (planes[:lay.w_total].double(), planes[lay.w_total:].double())
    else:
        assert w.numel() == lay.w_total and b.numel() == lay.b_total
        planes = (w.double(),)
    for i in range(len(lay.conv)):
        d = lay.conv[i]
        mats = []
        for pl in planes:
            blk = pl[d.w_off:d.w_off + d.cout * d.k_padded]
            if split and i >= 1:          # K-tile-major: element (n, k) at ((k / 32) * cout + n) * 32 + k % 32
                blk = blk.view(d.k_padded // 32, d.cout, 32).permute(1, 0, 2).reshape(d.cout, d.k_padded)
            else:
                blk = blk.view(d.cout, d.k_padded)
            assert float(blk[:, d.k * d.k * d.cin:].abs().sum()) == 0.0          # the K padding of conv 0
            mats.append(blk[:, :d.k * d.k * d.cin].reshape(d.cout, d.k, d.k, d.cin).permute(0, 3, 1, 2).contiguous())
        ops.whi.append(mats[0])
        ops.wlo.append(mats[1] if split else None)
        ops.w.append(mats[0] + mats[1] if split else mats[0])
        ops.b.append(b[d.b_off:d.b_off + d.cout].double())
        ops.cs.append(b[lay.b_total + d.b_off:lay.b_total + d.b_off + d.cout].double() if split else torch.ones(d.cout, dtype=torch.float64))
        ops.desc.append((d.cin, d.cout, d.k, d.stride, d.pad))
    return ops


@functools.lru_cache(maxsize=None)
def operands(mode, weights):
    return decode(mode, *packed(mode, weights))


def operands_from_state_dict(sd):
    """The same structure folded from a state dict in float64 without any rounding (test a of the host test)."""
    ops = Operands()
    lay = rn.resnet50_layout()
    for i, (cn, bn) in enumerate(rn.conv_names()):
        d = lay.conv[i]
        cw = sd[cn + ".weight"].double()
        scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + ro.BN_EPS)
        ops.w.append(cw * scale.view(-1, 1, 1, 1))
        ops.whi.append(ops.w[-1])
        ops.wlo.append(None)
        ops.b.append(sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale)
        ops.cs.append(torch.ones_like(scale))
        assert tuple(cw.shape) == (d.cout, d.cin, d.k, d.k)
        ops.desc.append((d.cin, d.cout, d.k, d.stride, d.pad))
    return ops


def conv_index(k):
    """Index of block k's reduce 1x1 in the conv order; then +1 the 3x3, +2 the expand, +3 the downsample (first blocks)."""
    i = 1
    for li, b in BLOCKS[:k]:
        i += 4 if b == 0 else 3
    return i


# ---- the emulation --------------------------------------------------------------------------------------------------------

def _cvt(v, fmt):
    return v.to(fmt).to(v.dtype)


def _split(v, fmt):
    hi = _cvt(v, fmt)
    return hi, _cvt(v - hi, fmt)


class Emu:
    """The block arithmetic of one numeric mode.  prec = torch.float64: the reference (joined operands, exact products);
    prec = torch.float32: the same on the CPU in float32 (split modes: three float32 products) -- the reference's floor.
    mode = None: no rounding anywhere (test a).  Activations are NHWC tensors of `prec`.
    `mutate`: {(conv index, stage): fn} hooks of the host test's injected mistakes."""

    def __init__(self, mode, ops, prec=torch.float64, mutate=None):
        self.mode, self.ops, self.prec, self.mutate = mode, ops, prec, mutate or {}
        self.fmt = {"f16x3": torch.float16, "bf16x3": torch.bfloat16}.get(mode)

    def q(self, v):
        if self.mode in (None, "fp32"):
            return v
        if self.mode == "bf16":
            return _cvt(v, torch.bfloat16)
        hi, lo = _split(v, self.fmt)
        return hi + lo

    def _product(self, a, wt, k, stride, pad):
        if k == 1:
            a = a[:, ::stride, ::stride]
            return (a.reshape(-1, a.shape[-1]) @ wt.reshape(wt.shape[0], -1).t()).view(*a.shape[:3], wt.shape[0])
        return F.conv2d(a.permute(0, 3, 1, 2), wt, stride=stride, padding=pad).permute(0, 2, 3, 1)

    def conv(self, i, a, relu):
        """act(conv_i(a) * cs + b), not yet rounded."""
        cin, cout, k, stride, pad = self.ops.desc[i]
        o, p = self.ops, self.prec
        pre = self.mutate.get((i, "input"))
        prod = lambda x, wt: self._product(pre(x) if pre else x, wt.to(p), k, stride, 0 if pre else pad)
        if self.fmt is not None and p != torch.float64:
            hi, lo = _split(a, self.fmt)
            acc = prod(hi, o.whi[i]) + prod(hi, o.wlo[i]) + prod(lo, o.whi[i])
        else:
            acc = prod(a, o.w[i])
        post = self.mutate.get((i, "acc"))
        if post:
            acc = post(self, i, a, acc)
        v = acc * o.cs[i].to(p) + o.b[i].to(p)
        return torch.relu(v) if relu else v

    def stem(self, x_nchw, parts=False):
        """x: normalised fp32 NCHW -> the pooled stem output NHWC (parts: also conv1's map)."""
        a = self.q(x_nchw.to(self.prec).permute(0, 2, 3, 1))
        c = self.conv(0, a, True)
        post = self.mutate.get((0, "map"))
        if post:
            c = post(c)
        pooled = self.q(F.max_pool2d(c.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
        return (pooled, c) if parts else pooled

    def t1(self, k, x):
        return self.q(self.conv(conv_index(k), x.to(self.prec), True))

    def y(self, k, x, t1):
        ci = conv_index(k)
        x, t1 = x.to(self.prec), t1.to(self.prec)
        t2 = self.q(self.conv(ci + 1, t1, True))
        post = self.mutate.get((ci + 1, "out"))
        if post:
            t2 = post(self, ci + 1, t1, t2)
        idn = self.q(self.conv(ci + 3, x, False)) if BLOCKS[k][1] == 0 else x
        return self.q(torch.relu(self.conv(ci + 2, t2, False) + idn))

    @staticmethod
    def features(y):
        """[n, 2048]: the mean of the top-left 7 x 7 of the final map."""
        return y[:, :7, :7].sum(dim=(1, 2)) / 49.0

    def chain(self, x_nchw, start=None):
        """Every tap from the emulation's own earlier taps (not teacher-forced): list of 33 NHWC tensors.
        start = (k, taps): keep taps before block k and continue from there."""
        if start is None:
            taps, k0 = [self.stem(x_nchw)], 0
        else:
            k0, taps = start[0], list(start[1][:1 + 2 * start[0]])
        for k in range(k0, len(BLOCKS)):
            x = taps[2 * k]
            taps.append(self.t1(k, x))
            taps.append(self.y(k, x, taps[-1]))
        return taps


def as_taps(flat, offsets, n, H, W):
    """The hook's flat fp32 buffer -> list of 33 NHWC tensors (views)."""
    shapes = tap_shapes(n, H, W)
    out = []
    for i, s in enumerate(shapes):
        assert offsets[i + 1] - offsets[i] == int(np.prod(s)), (i, s)
        out.append(flat[offsets[i]:offsets[i + 1]].view(*s))
    return out


def teacher_forced(emu, taps, x_nchw, which=None):
    """Reference of every tap (or of those in `which`) from the earlier TAPS: dict tap index -> tensor of emu.prec."""
    ref = {}
    want = range(N_TAPS) if which is None else which
    with oracle_threads(), torch.no_grad():
        for i in want:
            if i == 0:
                ref[0] = emu.stem(x_nchw)
            elif i % 2:
                ref[i] = emu.t1((i - 1) // 2, taps[i - 1])
            else:
                k = (i - 2) // 2
                ref[i] = emu.y(k, taps[i - 2], taps[i - 1])
    return ref


@functools.lru_cache(maxsize=None)
def stem_reference(row_id, mode, weights):
    """The one reference that does not depend on the taps: cached per row, emulation and weight set (both input forms share it)."""
    with oracle_threads(), torch.no_grad():
        return Emu(mode, operands(mode, weights)).stem(normalised(row_id))


@functools.lru_cache(maxsize=None)
def host_chain(row_id, mode, weights):
    """The float32 CPU evaluation of the emulation, chained on its own taps: the stand-in for the HIP path in the host test."""
    with oracle_threads(), torch.no_grad():
        return Emu(mode, operands(mode, weights), prec=torch.float32).chain(normalised(row_id))


# ---- the criterion ---------------------------------------------------------------------------------------------------------

def measure(got, ref):
    """dict(ratio, index, got, ref, rms, unequal): the worst element of |got - ref| / (|ref| + rms) and the share of elements
    that differ at all."""
    got, ref = got.double(), ref.double()
    rms = float(ref.pow(2).mean().sqrt())
    d = (got - ref).abs()
    ratio = d / (ref.abs() + max(rms, 1e-300))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    j = int(ratio.argmax())
    idx = tuple(int(v) for v in np.unravel_index(j, tuple(ratio.shape)))
    return dict(ratio=float(ratio.reshape(-1)[j]), index=idx, got=float(got.reshape(-1)[j]), ref=float(ref.reshape(-1)[j]), rms=rms,
                unequal=float((d != 0).double().mean()), rows=d.reshape(-1, d.shape[-1]).amax(dim=1))


def where(name, m):
    """Failure text: the tap, the worst index, both values and the three worst rows (pixels)."""
    rows = [int(r) for r in torch.argsort(m["rows"], descending=True)[:3]]
    return (f"{name}: worst at {m['index']}: got {m['got']:.9g} ref {m['ref']:.9g} (ratio {m['ratio']:.3e}, rms {m['rms']:.3g}, "
            f"unequal {m['unequal']:.4%}); worst rows {rows} of {m['rows'].numel()}")


def violations(mode, taps, ref, weights="std"):
    """List of failure texts of the taps in `ref` against the criterion of `mode`."""
    bad = []
    for i, rf in ref.items():
        m = measure(taps[i], rf)
        r = bound(mode, weights)[tap_kind(i)]
        if not m["ratio"] <= r:
            bad.append(where(f"tap {i} {tap_name(i)} > r = {r:.3e}", m))
        elif mode == "bf16" and m["unequal"] > BF16_UNEQUAL_CAP:
            bad.append(where(f"tap {i} {tap_name(i)}: more than {BF16_UNEQUAL_CAP:.0%} of the elements differ from the rounded reference", m))
    return bad


# ---- the HIP path (GPU test and its worker) -----------------------------------------------------------------------------------

GUARD = 256


def tap_offsets(n, H, W):
    """The hook's own offset table (taps == NULL: nothing is launched)."""
    import ctypes
    off = (ctypes.c_int64 * 34)()
    z = _lib.ptr(None)
    _lib.check(_lib.lib().sq_dbg_resnet50_taps(_lib.SQ_F32, z, z, z, z, n, H, W, z, z, 0, z, z, z, 0, off))
    return [int(v) for v in off]


def run_taps(mode, weights, row_id, form="u8", short_by=0, shape=None):
    """One forward through sq_dbg_resnet50_taps on cuda:0: (taps: list of 33 NHWC fp32 CPU tensors, features [n, 2048] CPU).
    form: "u8" (uint8 NHWC, fused normalisation) or "f32" (normalised fp32 NCHW).  short_by / shape: the refusal tests."""
    import ctypes
    r = BY_ID[row_id]
    n, H, W = r["n"], r["H"], r["W"]
    dev = torch.device("cuda:0")
    dt = _lib.DTYPES[mode]
    w, b = (t.to(dev) for t in packed(mode, weights))
    u8 = torch.from_numpy(patches(row_id)).to(dev) if form == "u8" else None
    f32 = normalised(row_id).to(dev) if form == "f32" else None
    cH, cW = shape or (H, W)
    L = _lib.lib()
    need = L.sq_resnet50_workspace_bytes_hw(dt, n, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    off = (ctypes.c_int64 * 34)()
    total = tap_offsets(n, H, W)[33]
    assert total == sum(int(np.prod(s)) for s in tap_shapes(n, H, W))
    flat = torch.full((total + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    feats = torch.full((n, 2048), float("nan"), dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.sq_dbg_resnet50_taps(dt, _lib.ptr(w), _lib.ptr(b), _lib.ptr(u8), _lib.ptr(f32), n, cH, cW, _lib.ptr(feats), _lib.ptr(ws),
                                          ws.numel(), _lib.ptr(flag), _lib.stream_ptr(dev), _lib.ptr(flat), total - short_by, off))
    torch.cuda.synchronize()
    flat = flat.cpu()
    assert bool(torch.isnan(flat[total:]).all()), "the hook wrote behind its last tap"
    assert bool(torch.isfinite(flat[:total]).all()), "a tap holds a non-finite value or was not written"
    assert int(flag.item()) == 0
    return as_taps(flat, [int(v) for v in off], n, H, W), feats.cpu()


def check_forward(mode, weights, row_id, taps, feats, ref=None):
    """Every tap and the features of one HIP forward against the criterion: list of failure texts."""
    if ref is None:
        ref = teacher_forced(Emu(mode, operands(mode, weights)), taps, None, which=range(1, N_TAPS))
        ref[0] = stem_reference(row_id, mode, weights)
    assert sorted(ref) == list(range(N_TAPS))
    bad = violations(mode, taps, ref, weights)
    want = Emu.features(taps[-1].double())
    err = float((feats.double() - want).abs().max() / want.abs().max())
    if not err <= FEATURE_TOL:
        bad.append(f"features vs the mean of the last y tap: {err:.3e} > {FEATURE_TOL:.0e}")
    return bad
