"""Shared by tests/test_he2rna_prims_host.py and tests/test_gpu_he2rna_prims.py: the case tables, seeded inputs, references and
bounds of the HE2RNA device primitives taken alone (csrc/he2rna.hip, csrc/he2rna_train.hip).  Not a test module.  Everything here
runs on the CPU; references are computed once per row (lru_cache) and never modified.

Top-k mean (sq_he2rna_topk_mean, _bwd, sq_he2rna_window_topk_mean, sq_he2rna_loss_head).  Reference, float64 with autograd:
    s     = scores.double() * mask[..., None]
    t     = torch.sort(s, dim=1, descending=True, stable=True).values      # smaller tile index first among equals, +0 == -0
    out_k = (t[:, :k] * mask[:, :k, None]).sum(1) / mask[:, :k].sum(1, keepdim=True)
    pred  = sum over ks, in list order, of float32(scale) * out_k
and the gradient is autograd of (pred * grad_out.double()).sum() with respect to scores.  Bounds (derived, not measured):
    prediction  |got - ref| <= (n_ks + 3) * 2^-24 * sum_i |scale * out_{k_i}| + 2^-40 * max|s|   -- one fp32 rounding of acc / cnt and
                one of the product with scale per term, at most n_ks more in the running fp32 sum (the bound also holds when the
                compiler fuses product and sum into one fma: one rounding fewer); the fp64 sums of at most 128 terms are covered by
                the last summand.  NaN exactly where the reference is NaN.
    gradient    |got - ref| <= 2^-23 * |ref|  -- one fp32 rounding of d * grad_out, then a product with 0 or 1; exactly 0 where the
                reference is exactly 0, NaN exactly where it is NaN.
    loss        relative 2^-22 against float64 mean((pred_got - target)^2) of the kernel's own pred.
`topk_emulate` restates the kernel's arithmetic on the CPU (ranks by counting, fp64 sums in tile order, the fp32 roundings of
he2rna_topk_kernel, with and without the fma); the host test holds it to these bounds on every row.

sq_he2rna_tile_mask: torch on the CPU in float32, (x.max(dim=1).values > 0).float().  NaN features are outside the contract
(fmaxf drops a NaN, torch's max propagates it) and are not tested.

sq_he2rna_dropout: Philox4x32-10 restated in numpy (`philox4x32_10`, pinned to three known answers by the host test): element
(row, column) draws word column % 4 of the block with key (seed low, seed high) and counter (column / 4, row, layer, step);
u = (word >> 8) * 2^-24; kept when u >= float32(p) and then fl32(x * fl32(1 / (1 - p))), else +0.0.  Every byte equal.
sq_he2rna_dropout_gate: act > 0 ? fl32(grad * inv_keep) : +0.0 -- a select, so inf and NaN gradients of dropped units give 0."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import he2rna_oracle as ho  # noqa: E402

MAX_N, MAX_KS = 128, 16                  # HE_MAX_N, HE_MAX_KS of csrc/he2rna.h
ALL_KS = [1, 2, 5, 10, 20, 50, 100]
SIXTEEN = [16, 1, 2, 3, 5, 7, 8, 9, 11, 13, 15, 4, 6, 10, 12, 14]
SENTINEL = -12345.0
POISON = 3e38                            # columns >= G of a score table: a kernel that reads them is far off every bound
SENT_BITS = int(np.float32(SENTINEL).view(np.int32))


def up8(n):
    return (n + 7) // 8 * 8


# ----------------------------------------------------------------------------------------------------------------------
# top-k mean: reference, bounds, emulation
# ----------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("own_mask", "cnt_all", "rank_le_k", "ties_larger_first", "unzeroed")


def topk_ref(scores, mask, ks, scale, grad_out=None, mutate=None, round_scale=True):
    """scores f32 [B, N, G], mask f32 [B, N] -> dict(pred f64 [B, G], bound f64 [B, G], grad f64 [B, N, G] or None).
    `mutate` (one of MUTATIONS) gives a deliberately wrong reference for the host test's teeth."""
    assert mutate is None or mutate in MUTATIONS
    sc = float(np.float32(scale)) if round_scale else float(scale)
    x = scores.double().clone().requires_grad_(grad_out is not None)
    m = mask.double()
    s = x if mutate == "unzeroed" else x * m[..., None]
    if mutate == "ties_larger_first":
        t, idx = torch.sort(s.flip(1), dim=1, descending=True, stable=True)
        idx = s.shape[1] - 1 - idx
    else:
        t, idx = torch.sort(s, dim=1, descending=True, stable=True)
    weight = m[..., None].expand_as(s)
    if mutate == "own_mask":
        weight = torch.gather(weight, 1, idx)
    pred, mag = 0.0, 0.0
    for k in ks:
        k = int(k)
        kk = min(k + 1, s.shape[1]) if mutate == "rank_le_k" else k
        den = m.sum(1, keepdim=True) if mutate == "cnt_all" else m[:, :k].sum(1, keepdim=True)
        out_k = (t[:, :kk] * weight[:, :kk]).sum(1) / den
        pred = pred + sc * out_k
        mag = mag + (sc * out_k).detach().abs()
    grad = None
    if grad_out is not None:
        (pred * grad_out.double()).sum().backward()
        grad = x.grad.detach()
    smax = float((scores.double() * m[..., None]).abs().max())
    bound = (len(ks) + 3) * 2.0 ** -24 * mag + 2.0 ** -40 * smax
    return dict(pred=pred.detach(), bound=bound, grad=grad)


def topk_emulate(scores, mask, ks, scale, grad_out=None, fma=False):
    """The arithmetic of he2rna_topk_kernel on the CPU: s = fl32(score * mask); rank = entries that are larger plus equal ones with a
    smaller tile index (counted, never sorted); acc_i = fp64 sum over the tiles in ascending order of s * mask[rank] where
    rank < k_i; pred += fl32(acc_i / cnt_i) * scale in fp32, list order (`fma`: product and sum rounded once); gradient
    fl32(d * grad_out) * mask[n] with d the fp64 sum over i of scale * mask[rank] / cnt_i.  -> (pred f32 [B, G], grad f32 or None)."""
    s = (scores.numpy() * mask.numpy()[:, :, None]).astype(np.float32)
    B, N, G = s.shape
    tile = np.arange(N)[None, :, None]
    rank = np.zeros((B, N, G), dtype=np.int64)
    for m in range(N):
        u = s[:, m:m + 1, :]
        rank += (u > s) | ((u == s) & (m < tile))
    w = mask.numpy().astype(np.float64)
    wr = np.take_along_axis(np.broadcast_to(w[:, :, None], rank.shape), rank, axis=1)
    sc32 = np.float32(scale)
    pred = np.zeros((B, G), dtype=np.float32)
    d = np.zeros((B, N, G), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in ks:
            cnt = np.cumsum(w, axis=1)[:, int(k) - 1][:, None]                                          # [B, 1]
            acc = np.cumsum(np.where(rank < k, s.astype(np.float64) * wr, 0.0), axis=1)[:, -1, :]       # sequential, tile order
            q = (acc / cnt).astype(np.float32)
            if fma:
                pred = (q.astype(np.float64) * np.float64(sc32) + pred.astype(np.float64)).astype(np.float32)
            else:
                pred = pred + q * sc32
            d = d + np.where(rank < k, np.float64(sc32) * wr / cnt[:, :, None], 0.0)
        grad = None
        if grad_out is not None:
            go = grad_out.numpy().astype(np.float64)[:, None, :]
            grad = (d * go).astype(np.float32) * mask.numpy()[:, :, None]
    return torch.from_numpy(pred), (None if grad is None else torch.from_numpy(grad))


def check_pred(got, ref):
    """-> (worst |got - ref| / bound over the finite elements, list of complaints)."""
    got, want, bound = got.double(), ref["pred"], ref["bound"]
    bad = []
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        bad.append(f"NaN at {int((torch.isnan(got) != nan).sum())} positions where the reference differs")
    ok = ~nan & ~torch.isnan(got)
    if not bool(ok.any()):
        return 0.0, bad
    ratio = ((got - want).abs() / bound)[ok]
    worst = float(ratio.max())
    if not worst <= 1.0:
        bad.append(f"prediction off the bound: worst ratio {worst:.3e} at {int((ratio > 1).sum())} elements")
    return worst, bad


def check_grad(got, ref_grad):
    """-> (worst |got - ref| / (2^-23 |ref|) over the nonzero finite elements, list of complaints)."""
    got, want = got.double(), ref_grad
    bad = []
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        bad.append(f"NaN at {int((torch.isnan(got) != nan).sum())} positions where the reference differs")
    zero = want == 0
    if not bool((got[zero] == 0).all()):
        bad.append(f"{int((got[zero] != 0).sum())} elements nonzero where the reference is exactly 0")
    ok = ~nan & ~zero & ~torch.isnan(got)
    if not bool(ok.any()):
        return 0.0, bad
    ratio = ((got - want).abs() / (2.0 ** -23 * want.abs()))[ok]
    worst = float(ratio.max())
    if not worst <= 1.0:
        bad.append(f"gradient off the bound: worst ratio {worst:.3e} at {int((ratio > 1).sum())} elements")
    return worst, bad


def loss_reference(pred_got, target):
    """float64 mean((pred_got - target)^2) of the kernel's own prediction; the relative bound is LOSS_RTOL."""
    return float(((pred_got.double() - target.double()) ** 2).mean())


LOSS_RTOL = 2.0 ** -22


# ----------------------------------------------------------------------------------------------------------------------
# top-k mean: the table
# ----------------------------------------------------------------------------------------------------------------------
NS = (1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 100, 127, 128)
GS = (1, 127, 128, 129, 255, 256, 257, 300)
G_FOR_EVERY_N, N_FOR_EVERY_G = (1, 129, 257), (9, 128)
KS_KINDS = ("k1", "kN", "repeat", "sixteen", "unsorted", "seven")
VALUE_KINDS = ("gauss", "quant", "zeros", "const", "neg")
MASK_KINDS = ("none", "mid_end", "first", "first2", "all")
LD_KINDS = ("tight", "plus3", "pad")
SCALES = ("one", "mean", "0.3")


def _ks_of(kind, N):
    return {"k1": [1], "kN": [N], "repeat": [5, 5, 2], "sixteen": SIXTEEN, "unsorted": [20, 1, 5], "seven": ALL_KS}[kind]


def _ks_kinds_for(N):
    return [k for k, need in zip(KS_KINDS, (1, 1, 5, 16, 20, 100)) if N >= need]


def _ld_of(kind, G):
    return {"tight": G, "plus3": G + 3, "pad": up8(G) + 8}[kind]


def _scale_of(kind, ks):
    return {"one": 1.0, "mean": 1.0 / len(ks), "0.3": 0.3}[kind]


def _build_rows():
    """Every N meets G in {1, 129, 257}, every G meets N in {9, 128}; the other attributes go round by least use, so that every
    kind of ks, values, mask, leading dimension, scale and batch occurs (the host test counts them).  Rows with a name of their
    own behind them: the NaN patterns, the teeth of the host test and the unaligned base pointer."""
    pairs = sorted({(N, G) for N in NS for G in G_FOR_EVERY_N} | {(N, G) for G in GS for N in N_FOR_EVERY_G})
    used = {}

    def pick(group, options):
        c = used.setdefault(group, {})
        best = min(options, key=lambda o: (c.get(o, 0), options.index(o)))
        c[best] = c.get(best, 0) + 1
        return best

    rows = []
    for i, (N, G) in enumerate(pairs):
        kk = pick("ks", _ks_kinds_for(N))
        values = pick("values", [v for v in VALUE_KINDS if v != "neg" or N >= 2])
        mask = "mid_end" if values == "neg" else pick("mask", ["none", "mid_end"] if N >= 2 else ["none"])
        rows.append(dict(id=f"n{N}-g{G}", B=pick("B", [1, 3]), N=N, G=G, ks_kind=kk, ks=_ks_of(kk, N), values=values, mask=mask,
                         ld_kind=pick("ld", list(LD_KINDS)), scale_kind=pick("scale", list(SCALES)), off=0, seed=1000 + i))
    named = [
        # exact live ties in every column, tiles masked in the middle and at the end, k < N, the base pointer one float off 16 bytes
        dict(id="ties-n128-g257-off1", B=3, N=128, G=257, ks_kind="unsorted", values="quant", mask="mid_end", ld_kind="plus3", scale_kind="0.3", off=1),
        dict(id="ties-n17-g129", B=3, N=17, G=129, ks_kind="repeat", values="quant", mask="mid_end", ld_kind="tight", scale_kind="mean", off=0),
        # tile 4 of slide 0 is masked and k = 5 reaches it: the position's mask and the selected tile's own mask differ
        dict(id="mid-masked-n9-g257", B=3, N=9, G=257, ks_kind="repeat", values="gauss", mask="mid_end", ld_kind="pad", scale_kind="one", off=0),
        # slide B - 1 starts with a masked tile: k = 1 alone is 0/0, so its prediction is NaN; the other slides are finite
        dict(id="first-masked-n9-g129", B=3, N=9, G=129, ks_kind=None, ks=[1, 5], values="gauss", mask="first", ld_kind="pad", scale_kind="mean", off=0),
        # the same slide with k = 1 alone (a NaN row of the prediction) and with k = 5 alone (finite: position 0 weighs nothing)
        dict(id="first-masked-k1-n9-g129", B=3, N=9, G=129, ks_kind="k1", values="gauss", mask="first", ld_kind="tight", scale_kind="one", off=0),
        dict(id="first-masked-k5-n9-g129", B=3, N=9, G=129, ks_kind=None, ks=[5], values="gauss", mask="first", ld_kind="tight", scale_kind="one", off=0),
        # mask [0, 0, 1, 1, 0, 1, 1], ks [2, 4]: the prediction is NaN, the gradient NaN at ranks 0 and 1 (masked entries too), finite elsewhere
        dict(id="first2-n7-g129", B=1, N=7, G=129, ks_kind=None, ks=[2, 4], values="gauss", mask="first2", ld_kind="plus3", scale_kind="mean", off=0),
        dict(id="all-masked-n17-g257", B=3, N=17, G=257, ks_kind=None, ks=[1, 17], values="gauss", mask="all", ld_kind="tight", scale_kind="one", off=0),
        # every live score negative: the masked zeros outrank all of them
        dict(id="neg-n65-g129", B=3, N=65, G=129, ks_kind="unsorted", values="neg", mask="mid_end", ld_kind="pad", scale_kind="one", off=0),
        dict(id="zeros-n16-g129", B=3, N=16, G=129, ks_kind="sixteen", values="zeros", mask="mid_end", ld_kind="plus3", scale_kind="mean", off=0),
        dict(id="const-n100-g257", B=1, N=100, G=257, ks_kind="seven", values="const", mask="mid_end", ld_kind="pad", scale_kind="mean", off=0),
    ]
    for j, r in enumerate(named):
        if r["ks_kind"] is not None:
            r["ks"] = _ks_of(r["ks_kind"], r["N"])
        r["seed"] = 2000 + j
        rows.append(r)
    for r in rows:
        r["ld"] = _ld_of(r["ld_kind"], r["G"])
        r["scale"] = _scale_of(r["scale_kind"], r["ks"])
    return rows


TOPK_ROWS = _build_rows()
TOPK_BY_ID = {r["id"]: r for r in TOPK_ROWS}
NAN_ROWS = ("first-masked-n9-g129", "first-masked-k1-n9-g129", "first2-n7-g129", "all-masked-n17-g257")      # 0/0 in some slide
# the rows the host test's mutations must break (prediction, or gradient for the tie rule)
TEETH_ROWS = {"own_mask": "mid-masked-n9-g257", "cnt_all": "ties-n17-g129", "rank_le_k": "ties-n17-g129",
              "ties_larger_first": "ties-n128-g257-off1", "unzeroed": "neg-n65-g129"}


def _values(kind, B, N, width, gen):
    x = torch.randn(B, N, width, generator=gen)
    if kind == "quant":
        x = torch.round(x * 6) / 4                                           # multiples of 0.25: exact ties in every long column
    elif kind == "zeros":
        z = torch.randint(0, 4, (B, N, width), generator=gen)
        x = torch.where(z == 0, torch.tensor(0.0), x)
        x = torch.where(z == 1, torch.tensor(-0.0), x)
    elif kind == "const":
        x = x[:, :1, :].expand(B, N, width).clone()
    elif kind == "neg":
        x = -(x.abs() + 0.1)
    return x


def _mask(kind, B, N):
    m = torch.ones(B, N)
    if kind == "mid_end":
        if N >= 7:
            m[0, N // 2] = 0
            m[0, N - 1] = 0
            m[B - 1, N - 3:] = 0
        else:
            m[0, N - 1] = 0
    elif kind == "first":
        m[B - 1, 0] = 0
    elif kind == "first2":
        m[0, 0] = m[0, 1] = m[0, 4] = 0
    elif kind == "all":
        m[B // 2] = 0
    return m


@functools.lru_cache(maxsize=None)
def topk_inputs(rid):
    """dict(scores f32 [B, N, ld] with POISON in the columns >= G, mask f32 [B, N], grad_out f32 [B, G] (0.5 <= |.| < 1.5),
    target f32 [B, G])."""
    r = TOPK_BY_ID[rid]
    gen = torch.Generator().manual_seed(r["seed"])
    B, N, G, ld = r["B"], r["N"], r["G"], r["ld"]
    scores = _values(r["values"], B, N, ld, gen)
    scores[:, :, G:] = POISON
    sign = torch.where(torch.rand(B, G, generator=gen) < 0.5, -1.0, 1.0)
    return dict(scores=scores, mask=_mask(r["mask"], B, N), grad_out=sign * (0.5 + torch.rand(B, G, generator=gen)),
                target=torch.rand(B, G, generator=gen) * 3)


@functools.lru_cache(maxsize=None)
def topk_reference(rid, mutate=None):
    r, q = TOPK_BY_ID[rid], topk_inputs(rid)
    return topk_ref(q["scores"][:, :, :r["G"]], q["mask"], r["ks"], r["scale"], q["grad_out"], mutate)


def is_tie_free(rid):
    """Gaussian scores, no leading masked tile: torch.topk's own tie order cannot matter (the masked zeros tie only among
    themselves, and their gradient is zero whatever their order)."""
    r = TOPK_BY_ID[rid]
    return r["values"] == "gauss" and r["mask"] in ("none", "mid_end")


def oracle_inputs(scores, mask):
    """(state dict, x [B, G + 1, N], input_dim) that make oracle/he2rna_oracle.py see exactly these scores and this mask: channel 0
    carries the mask, channel 1 + g carries score g minus 64 (so a masked tile has no positive channel), and the one 1x1
    layer adds 64 * mask back.  Differentiable in `scores` (float64)."""
    B, N, G = scores.shape
    x = torch.cat([mask.double()[:, None, :], (scores - 64.0).transpose(1, 2)], dim=1)
    w = torch.cat([torch.full((G, 1), 64.0, dtype=torch.float64), torch.eye(G, dtype=torch.float64)], dim=1)[:, :, None]
    return {"conv0.weight": w, "conv0.bias": torch.zeros(G, dtype=torch.float64)}, x, G + 1


# ----------------------------------------------------------------------------------------------------------------------
# sliding windows
# ----------------------------------------------------------------------------------------------------------------------
GATHER_ROWS = 500
WIN_NS = (1, 7, 8, 9, 100, 127, 128)
WIN_GS = (1, 127, 128, 129, 300)
WIN_PAD_WINDOW = 5                       # of the 37-window rows: its first max(ks) slots are all padding


def _build_win_rows():
    rows, used = [], {}
    for i, (N, G) in enumerate((N, G) for N in WIN_NS for G in WIN_GS):
        kinds = _ks_kinds_for(N)
        c = used.setdefault(len(kinds), [0])
        kk = kinds[c[0] % len(kinds)]
        c[0] += 1
        ks = _ks_of(kk, N)
        rows.append(dict(id=f"w-n{N}-g{G}", N=N, G=G, n_windows=37 if (WIN_NS.index(N) + WIN_GS.index(G)) % 2 == 0 else 1, ks_kind=kk, ks=ks,
                         ld=_ld_of(LD_KINDS[i % 3], G), scale=_scale_of(SCALES[i % 3], ks), seed=3000 + i))
    return rows


WIN_ROWS = _build_win_rows()
WIN_BY_ID = {r["id"]: r for r in WIN_ROWS}


@functools.lru_cache(maxsize=None)
def win_inputs(rid):
    """dict(scores f32 [500, ld] Gaussian (POISON at columns >= G), mask f32 [500] with about one zero in seven, idx int32
    [n_windows, N]).  About 5 % of the indices are -1 and 5 % are at or beyond the table (500, 501, 2^31 - 1); every window of two or
    more tiles names one table row twice (live ties from ordinary data); window WIN_PAD_WINDOW starts with max(ks) padding slots."""
    r = WIN_BY_ID[rid]
    gen = torch.Generator().manual_seed(r["seed"])
    N, G, ld, nw = r["N"], r["G"], r["ld"], r["n_windows"]
    scores = torch.randn(GATHER_ROWS, ld, generator=gen)
    scores[:, G:] = POISON
    mask = (torch.rand(GATHER_ROWS, generator=gen) >= 1.0 / 7).float()
    idx = torch.randint(0, GATHER_ROWS, (nw, N), generator=gen, dtype=torch.int32)
    kind = torch.rand(nw, N, generator=gen)
    beyond = torch.tensor([GATHER_ROWS, GATHER_ROWS + 1, 2 ** 31 - 1], dtype=torch.int32)[torch.randint(0, 3, (nw, N), generator=gen)]
    if N >= 7:                                       # shorter windows keep their few slots (their pad window is all padding anyway)
        idx = torch.where(kind < 0.05, torch.tensor(-1, dtype=torch.int32), idx)
        idx = torch.where((kind >= 0.05) & (kind < 0.10), beyond, idx)
    if N >= 2:
        idx[:, N - 1] = idx[:, 0]
    if N >= 8:
        idx[:, 5] = idx[:, 2]
    if nw > WIN_PAD_WINDOW:
        idx[WIN_PAD_WINDOW, :max(r["ks"])] = torch.tensor([-1, GATHER_ROWS][N % 2], dtype=torch.int32)
    return dict(scores=scores, mask=mask, idx=idx.contiguous())


def materialise(scores, mask, idx, G):
    """The batch a window map stands for: (scores f32 [n_windows, N, G], mask f32 [n_windows, N]); an index outside [0, gather_rows)
    gives score 0 and mask 0."""
    ok = (idx >= 0) & (idx < scores.shape[0])
    safe = torch.where(ok, idx, torch.zeros_like(idx)).long()
    s = torch.where(ok[..., None], scores[safe][..., :G], torch.tensor(0.0))
    return s.contiguous(), torch.where(ok, mask[safe], torch.tensor(0.0)).contiguous()


@functools.lru_cache(maxsize=None)
def win_batch(rid):
    q = win_inputs(rid)
    return materialise(q["scores"], q["mask"], q["idx"], WIN_BY_ID[rid]["G"])


@functools.lru_cache(maxsize=None)
def win_reference(rid):
    r = WIN_BY_ID[rid]
    s, m = win_batch(rid)
    return topk_ref(s, m, r["ks"], r["scale"])


# ----------------------------------------------------------------------------------------------------------------------
# tile mask
# ----------------------------------------------------------------------------------------------------------------------
MASK_ROWS = (1, 3, 4, 5, 1027)
MASK_CS = (1, 2, 63, 64, 65, 129, 2048)
DENORM_MIN = np.float32(1e-45)           # the smallest positive denormal, bits 0x00000001
MASK_SPECIALS = ("all_negative", "all_pos_zero", "all_neg_zero", "positive_last", "positive_at_64", "denormal", "pos_inf", "all_neg_inf")


def tile_mask_specials(rows, C):
    """{row: kind}: the special rows of a [rows, C] case.  1027 rows hold every kind; the short tables take len(rows) kinds each,
    starting where the channel count's index says, so that every kind meets every C somewhere."""
    first = MASK_CS.index(C) * 3 + MASK_ROWS.index(rows)
    return {r: MASK_SPECIALS[(first + r) % len(MASK_SPECIALS)] for r in range(min(rows, len(MASK_SPECIALS)))}


@functools.lru_cache(maxsize=None)
def tile_mask_case(rows, C):
    """(x f32 [rows, C] numpy, expected mask f32 [rows] from torch on the CPU).  Ordinary rows are all negative, half of them with
    one positive value at a random channel."""
    rs = np.random.RandomState(rows * 10007 + C)
    x = -(np.abs(rs.randn(rows, C)) + 0.01).astype(np.float32)
    lit = rs.rand(rows) < 0.5
    x[np.flatnonzero(lit), rs.randint(0, C, int(lit.sum()))] = 0.5
    for r, kind in tile_mask_specials(rows, C).items():
        x[r] = -(np.abs(rs.randn(C)) + 0.01)
        if kind == "all_pos_zero":
            x[r] = 0.0
        elif kind == "all_neg_zero":
            x[r] = -0.0
        elif kind == "positive_last":
            x[r, C - 1] = 0.25
        elif kind == "positive_at_64":                                       # the second round of lane 0 when C = 65
            x[r, min(64, C - 1)] = 0.25
        elif kind == "denormal":
            x[r] = 0.0
            x[r, C // 2] = DENORM_MIN
        elif kind == "pos_inf":
            x[r, C // 3] = np.inf
        elif kind == "all_neg_inf":
            x[r] = -np.inf
    want = (torch.from_numpy(x).max(dim=1).values > 0).float().numpy()
    return x, want


# ----------------------------------------------------------------------------------------------------------------------
# Philox4x32-10, dropout, gate
# ----------------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _U32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11) on arrays: counter = four and key = two
    integers or integer arrays below 2^32 -> four uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(_U32) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(_U32) for v in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(_U32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(_U32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(_W0)) & np.uint64(_U32), (k[1] + np.uint64(_W1)) & np.uint64(_U32)]
    return c


PHILOX_KNOWN_ANSWERS = (        # the known-answer vectors of Random123 (kat_vectors, philox4x32 10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((_U32, _U32, _U32, _U32), (_U32, _U32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def dropout_keep(rows, width, p, seed, step, layer, mutate=None):
    """bool [rows, width]: which elements sq_he2rna_dropout keeps.  mutate: "swap_counter" exchanges the counter words (row,
    column / 4), "low_key" uses only the low key word -- the host test shows that either changes the pattern of a named case."""
    row = np.arange(rows, dtype=np.uint64)[:, None]
    col = np.arange(width, dtype=np.uint64)[None, :]
    seed &= (1 << 64) - 1
    k0, k1 = seed & _U32, (seed >> 32) if mutate != "low_key" else 0
    c0, c1 = (col // np.uint64(4), row) if mutate != "swap_counter" else (row, col // np.uint64(4))
    words = philox4x32_10((c0, c1, layer, step), (k0, k1))
    word = np.select([col % np.uint64(4) == np.uint64(j) for j in range(4)], [np.broadcast_to(w, (rows, width)) for w in words])
    u = ((word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return u >= np.float32(p)


def dropout_reference(x, p, seed, step, layer):
    """x f32 [rows, width] -> the table sq_he2rna_dropout leaves, bit for bit."""
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    keep = dropout_keep(x.shape[0], x.shape[1], p, seed, step, layer)
    return np.where(keep, (x * inv_keep).astype(np.float32), np.float32(0.0)).astype(np.float32)


def gate_reference(grad, act, p):
    """-> the gradient table sq_he2rna_dropout_gate leaves: act > 0 ? fl32(grad * inv_keep) : +0.0 (NaN > 0 is false)."""
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    with np.errstate(invalid="ignore"):
        return np.where(act > 0, (grad * inv_keep).astype(np.float32), np.float32(0.0)).astype(np.float32)


WIDTHS = (1, 3, 4, 5, 13, 64)
ELEM_ROWS = (1, 7, 300)
DROP_PS = (0.5, 0.1, 2.0 ** -24, 1.0 - 2.0 ** -24)
DROP_SEEDS = (0, 1234, 0x1234567800000001, -1)
DROP_LAYERS = (0, 3)
DROP_STEPS = (0, 2 ** 32 - 1)
GATE_PS = (0.0, 0.5, 0.1)


def elem_ld(kind, width):
    """tight: the width itself; pad: 16 floats, or a multiple of 8 beyond a wider table (16-byte rows), pad2 another one; odd: the next value that is no multiple of 4."""
    return {"tight": width, "pad": 16 if width <= 16 else up8(width) + 8, "pad2": up8(width) + 16, "odd": width + 1 if (width + 1) % 4 else width + 2}[kind]


def takes_vector_path(ld, off):
    return ld % 4 == 0 and off % 4 == 0


def _build_dropout_cases():
    cases = []
    geoms = [(w, kind, off, rows) for w in WIDTHS for kind in ("tight", "pad", "odd") for off in (0, 1) for rows in ELEM_ROWS]
    for i, (w, kind, off, rows) in enumerate(geoms):
        j = i * 37 % 64                                                      # 37 is odd: the 64 parameter combinations all occur
        cases.append(dict(id=f"d-w{w}-{kind}-off{off}-r{rows}", width=w, ld=elem_ld(kind, w), ld_kind=kind, off=off, rows=rows,
                          p=DROP_PS[j % 4], seed=DROP_SEEDS[j // 4 % 4], layer=DROP_LAYERS[j // 16 % 2], step=DROP_STEPS[j // 32],
                          data_seed=4000 + i))
    return cases


DROPOUT_CASES = _build_dropout_cases()
DROPOUT_BY_ID = {c["id"]: c for c in DROPOUT_CASES}
DROPOUT_TEETH_CASE = "d-w13-pad-off0-r7"
# (grad ld, act ld, grad offset, act offset): both tables aligned (16-byte accesses), then every way one of them forces the scalar path
GATE_GEOMS = (("pad", "pad2", 0, 0), ("tight", "pad", 0, 0), ("pad", "odd", 0, 0), ("odd", "pad", 0, 0), ("pad", "pad2", 1, 0),
              ("pad", "pad2", 0, 1))


def _build_gate_cases():
    cases = []
    for i, (w, geom, rows) in enumerate((w, g, r) for w in WIDTHS for g in GATE_GEOMS for r in ELEM_ROWS):
        kg, ka, og, oa = geom
        cases.append(dict(id=f"g-w{w}-{kg}{og}-{ka}{oa}-r{rows}", width=w, ld_grad=elem_ld(kg, w), ld_act=elem_ld(ka, w), off_grad=og,
                          off_act=oa, rows=rows, p=GATE_PS[(i + i // 3) % 3], data_seed=5000 + i))
    return cases


GATE_CASES = _build_gate_cases()


def embed(table, ld, off, guard=8):
    """A [rows, width] table inside a flat float32 buffer of SENTINEL: `off` floats in front, rows `ld` apart, `guard` behind.
    -> (flat numpy array, the [rows, width] view into it)."""
    rows, width = table.shape
    flat = np.full(off + rows * ld + guard, SENTINEL, dtype=np.float32)
    view = np.lib.stride_tricks.as_strided(flat[off:], shape=(rows, width), strides=(ld * 4, 4))
    view[...] = table
    return flat, view


def dropout_input(case):
    return np.random.RandomState(case["data_seed"]).randn(case["rows"], case["width"]).astype(np.float32)


def gate_inputs(case):
    """(grad, act) f32 [rows, width].  act: positive, negative, +0.0, -0.0, the smallest denormal and NaN; grad: Gaussian, and inf or
    NaN at two thirds of the positions whose unit is not kept."""
    rs = np.random.RandomState(case["data_seed"])
    shape = (case["rows"], case["width"])
    kind = rs.randint(0, 10, shape)
    act = (np.abs(rs.randn(*shape)) + 0.01).astype(np.float32)
    act[kind == 4] *= -1
    act[kind == 5] *= -1
    act[kind == 6] = 0.0
    act[kind == 7] = -0.0
    act[kind == 8] = DENORM_MIN
    act[kind == 9] = np.nan
    grad = rs.randn(*shape).astype(np.float32)
    bad = rs.randint(0, 3, shape)
    with np.errstate(invalid="ignore"):
        dropped = ~(act > 0)
    grad[dropped & (bad == 0)] = np.inf
    grad[dropped & (bad == 1)] = np.nan
    return grad, act
