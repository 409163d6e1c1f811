"""Case tables of the GEMM contract sweep, shared by tests/test_gemm_cases_host.py (CPU: is every row well conditioned, does
it reach the branch it names, would it catch the mistake it is there for?) and tests/test_gpu_gemm_contract.py (GPU:
sq_linear, sq_linear_weight_grad and sq_linear_weight_grad_group against float64).

Every row names the launch-code branch it is there for.  Operands come from a generator seeded by the row id and are
bf16-exact (gpu_util.to_bf16_f32), so the f32 and the bf16 run of a row share one float64 reference.  Rows with fewer than 64
output elements (and weight-gradient rows whose bias gradient has fewer than 64) use operands shifted positive: a one-element
result then cannot sit near zero and gpu_util.rel_err (max |diff| / max |ref|) keeps its meaning.

Buffers are built so that a mistake shows:
* operand padding -- columns [K, lda), [K, ldw), [NI, ldx), [round_up(NO, 8), lddy), the columns in front of a sub-view's
  offset and one row beyond M / N / T -- holds NaN: an over-read poisons the result;
* dY columns [NO, round_up(NO, 8)) hold zero, as every caller keeps them, except in the row that pins that they may hold
  anything (TN_DY_PAD_NAN, NaN there);
* output buffers are over-allocated and filled with a NaN bit pattern (SENT32 / SENT16); `judge` counts every element outside
  [0, M) x [0, N) whose bits changed -- columns [N, ldc), rows >= M, the elements in front of a column-offset base, the guard
  floats around dbias -- and an output element the kernel never wrote stays NaN and fails the error bound.

Tolerances are the project's (tests/test_gpu_gemm.py): f32 output 2e-6 (f32 operands also through the exact GELU), bf16
operands through the fast GELU 2e-3, bf16 output 5e-3 (1e-2 on the forced gemm_p8 / ring kernels), split-K 1e-5, weight
gradients 1e-5."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gpu_util import rel_err, to_bf16_f32

EPC = {"f32": 4, "bf16": 8}                 # elements per 16-byte chunk
SENT32, SENT16 = 0x7FA5C3E1, 0x7FA5         # NaN bit patterns of the output sentinels (int32 / int16 views)
FORCED_TILES = (11, 12, 21, 22)             # sq_dbg_set(0, t); 0 = the dispatch rule
NAN = float("nan")


def up(n, m):
    return (n + m - 1) // m * m


def _seed(s):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(s)) % 100003


def ld_of(mode, n):
    """An output / residual pitch: "N" contiguous, "vec" padded and 16-byte aligned, "odd" N + 3 (scalar epilogue)."""
    return {"N": n, "vec": up(n, 8) + 8, "odd": n + 3}[mode] if isinstance(mode, str) else mode


# ----------------------------------------------------------------------------------------------------------------------
# the launch rule of csrc/gemm.hip launch_t / launch_cfg, restated (the host test holds the branch rows to it)
# ----------------------------------------------------------------------------------------------------------------------
def nt_dispatch(dtype, M, N, K, ws_bytes=0, force_split=0):
    """-> dict(tile, splitk, per (K-tiles per slice), nk, one_buffer): what sq_linear launches for a plain product that
    neither gemm_p8.hip nor gemm_ring.hip takes (both need K >= 512 and hundreds of tiles)."""
    epc = EPC[dtype]
    blocks = lambda bm, bn: -(-M // bm) * -(-N // bn)
    can_split = ws_bytes > 0 and K >= 16 * 8 * epc
    nk = -(-K // (8 * epc))
    if N <= 64:
        tile = 21 if blocks(128, 64) >= 256 else 11
    elif M <= 64:
        tile = 12 if blocks(64, 128) >= 256 else 11
    elif nk <= 4 and blocks(128, 64) >= 1024:
        tile = 21
    elif blocks(128, 128) >= 256 or can_split:
        tile = 22
    else:
        tile = 11
    nb = blocks(tile // 10 * 64, tile % 10 * 64)
    splitk = 1
    if ws_bytes > 0 and N % 8 == 0 and nb < 256 and nk >= 4:
        s = min(-(-512 // nb), nk // 2, 32)
        while s > 1 and s * M * N * 4 > ws_bytes:
            s -= 1
        splitk = max(s, 1)
    if force_split > 0 and ws_bytes > 0 and N % 8 == 0:
        splitk = force_split
    return dict(tile=tile, splitk=splitk, per=-(-nk // splitk), nk=nk, one_buffer=nk == 1 and splitk == 1)


def last_slice_is_empty(nk, splitk):
    per = -(-nk // splitk)
    return splitk > 1 and (splitk - 1) * per >= nk


def tn_empty_slice_split(dtype, T):
    """The smallest sq_dbg_set(4, s) for which the last token slice of gemm_tn.hip's two-buffer kernel is empty."""
    nk = -(-T // (64 if dtype == "bf16" else 32))
    s = 2
    while not last_slice_is_empty(nk, s):
        s += 1
    return s


# ----------------------------------------------------------------------------------------------------------------------
# NT table (sq_linear)
# ----------------------------------------------------------------------------------------------------------------------
def _nt(id, M, N, K, family, branch, tags=(), **kw):
    """K: an int, or "epc" / "2epc" / "5tiles" (in units of the dtype's 16-byte chunk / 128-byte K-tile).  lda / ldw: "K" or
    "pad" (K + epc / K + 2 epc); a_off / w_off: column offset of the sub-view in chunks; ldc / ldres: see ld_of; c_off: column
    offset of C in elements; res: "none" / "f32" / "bf16"; ws: workspace bytes; split: sq_dbg_set(2, split)."""
    row = dict(id=id, M=M, N=N, K=K, family=family, branch=branch, tags=tuple(tags), lda="K", ldw="K", a_off=0, w_off=0, ldc="N",
               ldres="N", c_off=0, bias=True, res="f32", act=0, out="f32", ws=0, split=0, splits=False, dtypes=None)
    row.update(kw)
    return row


def nt_k(row, dtype):
    k = row["K"]
    return {"epc": EPC[dtype], "2epc": 2 * EPC[dtype], "5tiles": 40 * EPC[dtype]}[k] if isinstance(k, str) else k


def nt_dtypes(row):
    return row["dtypes"] or tuple(d for d in ("f32", "bf16") if nt_k(row, d) % EPC[d] == 0)


_LD3 = ("N", "vec", "odd")
# (75, 40, 48): two row tiles of 64, N = 40 = five whole 8-column chunks, K = 48 is 1.5 f32 / 0.75 bf16 K-tiles
NT_STRIDE = [
    _nt(f"nt-stride-ldc_{c}-ldres_{r}", 75, 40, 48, "stride", f"lda = K + epc, ldw = K + 2 epc, ldc {c}, ldres {r}",
        tags=("lda-padded", "ldw-padded", f"ldc-{c}", f"ldres-{r}"), lda="pad", ldw="pad", ldc=c, ldres=r,
        res="bf16" if (i + j) % 2 else "f32", act=(0, 2, 1)[j])
    for i, c in enumerate(_LD3) for j, r in enumerate(_LD3)
] + [
    _nt("nt-stride-a-w-subviews", 75, 40, 48, "stride", "A and W start one / two 16-byte chunks into a wider table",
        tags=("a-subview", "w-subview"), a_off=1, w_off=2, lda="pad", ldw="pad", act=2),
    _nt("nt-stride-c-offset1", 75, 40, 48, "stride", "C starts at column 1 of a wider table: misaligned base, scalar epilogue",
        tags=("c-offset-1",), c_off=1, ldc="vec", ldres="vec"),
    _nt("nt-stride-c-offset1-bf16out", 75, 40, 48, "stride", "the same with a bf16 output and a bf16 residual",
        tags=("c-offset-1",), c_off=1, ldc="vec", ldres="odd", res="bf16", out="bf16", act=2),
    _nt("nt-stride-c-offset4-f32", 75, 40, 48, "stride", "f32 C at column 4 (16 bytes) of a padded table: vector epilogue",
        tags=("c-offset-4-vector",), c_off=4, ldc="vec", ldres="vec", res="bf16"),
]


def _tiny(M, N, K, branch="", **kw):
    return _nt(f"nt-tiny-M{M}-N{N}-K{K}", M, N, K, "tiny", branch or f"tiny extents M {M}, N {N}, K {K}",
               tags=(f"M{M}", f"N{N}", f"K{K}") + tuple(kw.pop("tags", ())), act=kw.pop("act", (M + N) % 3), **kw)


NT_TINY = [
    _tiny(1, 1, "epc", "one output element, one 16-byte chunk of K"),
    _tiny(1, 1, 8),
    _tiny(2, 7, "2epc"),
    _tiny(65, 9, 36, "f32 only: K = 36 is one K-tile and one chunk; N = 9 one whole and one 1-column chunk"),
    # the reference's default HE2RNA (layers=[1]) at B N = 40 tiles, input_dim 32: hidden layer, then the output layer
    _tiny(40, 1, 32, "HE2RNA layers=[1], hidden layer: N = 1 written into rows of 8 columns, bias + ReLU", tags=("he2rna-n1",),
          ldc=8, res="none", act=2),
    _tiny(40, 12, 8, "HE2RNA layers=[1], output layer: K = 8 (the padded hidden width), G = 12 written into rows of 16",
          tags=("he2rna-k8",), ldc=16, res="none", act=0),
    _tiny(1, 2, 32), _tiny(1, 8, 64), _tiny(1, 63, 72), _tiny(1, 65, 36),
    _tiny(2, 1, 64), _tiny(2, 8, 72), _tiny(2, 9, "epc"), _tiny(2, 64, 32),
    _tiny(63, 1, 72), _tiny(63, 8, "2epc"), _tiny(63, 63, 32), _tiny(63, 65, 64),
    _tiny(64, 2, "epc"), _tiny(64, 7, 72), _tiny(64, 63, 36), _tiny(64, 64, 64),
    _tiny(65, 1, "epc"), _tiny(65, 7, 32), _tiny(65, 64, "2epc"), _tiny(65, 65, 72),
]

NT_BRANCH = [
    # N = 64 <= 64; blocks(128, 64) = 32768 / 128 * 1 = 256 >= 256 -> tile 21.  K = 16: one K-tile -> one LDS buffer
    _nt("nt-branch-tile21-narrow", 32768, 64, 16, "branch", "tile 21 by N <= 64 with 256 blocks", tags=("tile21-narrow",), want_tile=21),
    # N, M > 64; K-tiles = 64 / 32 = 2 (f32), 1 (bf16) <= 4; blocks(128, 64) = 32 * 32 = 1024 >= 1024 -> tile 21
    _nt("nt-branch-tile21-short-k", 4096, 2048, 64, "branch", "tile 21 by short K with 1024 blocks", tags=("tile21-short-k",), want_tile=21,
        act=2),
    # M = 64 <= 64; blocks(64, 128) = 1 * 32768 / 128 = 256 >= 256 -> tile 12
    _nt("nt-branch-tile12", 64, 32768, 64, "branch", "tile 12 by M <= 64 with 256 blocks", tags=("tile12",), want_tile=12, res="none"),
    # blocks(128, 64) = 3 * 3 = 9 < 1024, blocks(128, 128) = 6 < 256, no workspace -> tile 11; K = 32 is ONE f32 K-tile ->
    # launch_cfg takes a single operand buffer (16 KiB, the size of the fp32 epilogue stage)
    _nt("nt-branch-f32-one-buffer", 300, 136, 32, "branch", "fp32 one-buffer LDS form (K <= 32)", tags=("f32-one-buffer",), want_tile=11,
        want_one_buffer=True, act=1),
]

WS64 = 64 << 20
NT_SPLIT = [
    # 5 K-tiles in 4 forced slices: 2 tiles per slice, slice 3 starts at tile 6 > 5 -> empty, writes a zero partial
    _nt("nt-split-forced-empty-slice", 128, 128, "5tiles", "split", "sq_dbg_set(2, 4) over 5 K-tiles: the fourth slice is empty",
        tags=("split-forced-empty",), ws=WS64, split=4, splits=True, act=1),
    # f32: K = 512 >= 16 * 32 -> splittable; blocks(128, 128) = 8 * 13 = 104 < 256 -> tile 22; s = ceil(512 / 104) = 5 <= 16 / 2;
    # 5 slices x 6.5 MiB fit; 16 K-tiles / 5 -> 4 per slice: slices 0-3 hold all 16, the fifth is empty
    _nt("nt-split-natural-empty-slice", 1024, 1664, 512, "split", "5 slices of 4 K-tiles over 16: the fifth is empty",
        tags=("split-natural-empty",), ws=WS64, splits=True, act=1, dtypes=("f32",)),
    # one byte short of two slices: the slice count falls to 1, the plain kernel runs
    _nt("nt-split-workspace-one-byte-short", 1024, 1664, 512, "split", "a workspace one byte short of two slices: no split",
        tags=("split-workspace-short",), ws=2 * 1024 * 1664 * 4 - 1, act=2, dtypes=("f32",)),
    _nt("nt-split-n-not-multiple-of-8", 100, 68, 512, "split", "N % 8 = 4 with a workspace: not split", tags=("split-n-mod-8",),
        ws=WS64, act=2),
    # K = 1024: f32 tile 22, 2 blocks, 16 slices; bf16 tile 22, 8 slices.  The reduce kernel applies the epilogue
    _nt("nt-split-strided-vector-reduce", 96, 136, 1024, "split", "padded aligned ldc / ldres, GELU in the reduce kernel",
        tags=("split-strided-reduce",), ws=WS64, splits=True, act=1, ldc="vec", ldres="vec", lda="pad", ldw="pad"),
    _nt("nt-split-strided-scalar-reduce", 96, 136, 1024, "split", "ldc padded, bf16 residual at ldres = N + 3: scalar reduce epilogue, GELU",
        tags=("split-strided-reduce",), ws=WS64, splits=True, act=1, ldc="vec", ldres="odd", res="bf16"),
]

# the full product dtype x bias x residual x act x out runs over these two (looped inside one test each)
NT_EPI = [
    _nt("nt-epi-aligned", 200, 136, 96, "epi", "vector epilogue: every pitch a multiple of 16 bytes", tags=("epi-aligned",)),
    _nt("nt-epi-scalar-f32", 129, 65, 40, "epi", "scalar epilogue: ldc = ldres = 65", tags=("epi-scalar",), dtypes=("f32",)),
    _nt("nt-epi-scalar-bf16", 129, 65, 48, "epi", "scalar epilogue: ldc = ldres = 65", tags=("epi-scalar",), dtypes=("bf16",)),
]
EPI_PRODUCT = [dict(bias=b, res=r, act=a, out=o) for b in (False, True) for r in ("none", "f32", "bf16") for a in (0, 1, 2)
               for o in ("f32", "bf16")]

NT_SPECIAL = [
    _nt("nt-p8-549x512x328", 549, 512, 328, "p8", "forced gemm_p8 (tile 88), every pitch padded and 16-byte aligned", tags=("p8-strided",),
        lda="pad", ldw="pad", ldc="vec", ldres="vec", res="bf16", act=2, out="bf16", dtypes=("bf16",), tile=88),
    _nt("nt-p8-549x320x72", 549, 320, 72, "p8", "forced gemm_p8, K = 72: a K-tile with a single chunk, padded pitches", tags=("p8-strided",),
        lda="pad", ldw="pad", ldc="vec", ldres="vec", res="bf16", act=1, out="f32", dtypes=("bf16",), tile=88),
    _nt("nt-ring-aligned", 600, 256, 200, "ring", "forced ring kernel (tile 33), padded aligned pitches: the prefetching epilogue",
        tags=("ring-aligned",), lda="pad", ldw="pad", ldc="vec", ldres="vec", res="bf16", act=2, out="bf16", dtypes=("bf16",), tile=33),
    _nt("nt-ring-unaligned", 600, 256, 200, "ring", "forced ring kernel, ldc = ldres = N + 3 with a bf16 residual: sq_gemm_ring_eligible "
        "does not ask for aligned epilogue operands", tags=("ring-unaligned",), lda="pad", ldw="pad", ldc="odd", ldres="odd", res="bf16",
        act=2, out="bf16", dtypes=("bf16",), tile=33),
]

NT_ALL = NT_STRIDE + NT_TINY + NT_BRANCH + NT_SPLIT + NT_EPI + NT_SPECIAL
NT_BY_ID = {r["id"]: r for r in NT_ALL}
NT_REQUIRED_TAGS = (["lda-padded", "ldw-padded", "a-subview", "w-subview", "c-offset-1", "c-offset-4-vector", "he2rna-n1", "he2rna-k8"] +
                    [f"ldc-{c}" for c in _LD3] + [f"ldres-{c}" for c in _LD3] + [f"M{m}" for m in (1, 2, 63, 64, 65)] +
                    [f"N{n}" for n in (1, 2, 7, 8, 9, 63, 64, 65)] + [f"K{k}" for k in ("epc", "2epc", 32, 36, 64, 72)] +
                    ["tile21-narrow", "tile21-short-k", "tile12", "f32-one-buffer", "split-forced-empty", "split-natural-empty",
                     "split-workspace-short", "split-n-mod-8", "split-strided-reduce", "epi-aligned", "epi-scalar", "p8-strided",
                     "ring-aligned", "ring-unaligned"])


def nt_tol(dtype, r):
    if r["out"] == "bf16":
        return 1e-2 if r["family"] in ("p8", "ring") else 5e-3
    if r["splits"]:
        return 1e-5
    return 2e-3 if (r["act"] == 1 and dtype == "bf16") else 2e-6


@functools.lru_cache(maxsize=None)
def _nt_operands(case_id, dtype):
    row = NT_BY_ID[case_id]
    M, N, K = row["M"], row["N"], nt_k(row, dtype)
    g = torch.Generator().manual_seed(_seed(case_id))
    if M * N < 64:
        A, W = torch.rand(M, K, generator=g) + 0.5, (torch.rand(N, K, generator=g) + 0.5) / K
        bias, res = torch.rand(N, generator=g) + 0.5, torch.rand(M, N, generator=g) + 0.5
    else:
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) / math.sqrt(K) + torch.arange(N)[:, None] * 1e-3      # asymmetric rows
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    A, W, res = to_bf16_f32(A), to_bf16_f32(W), to_bf16_f32(res)
    return A, W, bias, res, A.double() @ W.double().T


def _act64(y, act):
    return F.gelu(y) if act == 1 else torch.relu(y) if act == 2 else y


def nt_problem(row, dtype, **over):
    """The host side of one sq_linear call: padded operand buffers (f32 tensors holding bf16-exact values and NaN), the
    geometry of the output buffer, the float64 reference and the tolerance.  `over` replaces epilogue fields of the row."""
    r = dict(row, **over)
    epc = EPC[dtype]
    M, N, K = r["M"], r["N"], nt_k(r, dtype)
    A, W, bias, res, prod = _nt_operands(row["id"], dtype)
    a0, w0 = r["a_off"] * epc, r["w_off"] * epc
    lda = a0 + K + (epc if r["lda"] == "pad" else 0)
    ldw = w0 + K + (2 * epc if r["ldw"] == "pad" else 0)
    A_buf = torch.full((M + 1, lda), NAN)
    A_buf[:M, a0:a0 + K] = A
    W_buf = torch.full((N + 1, ldw), NAN)
    W_buf[:N, w0:w0 + K] = W
    ldc, ldres = ld_of(r["ldc"], N), ld_of(r["ldres"], N)
    res_buf = None
    ref = prod
    if r["bias"]:
        ref = ref + bias.double()
    if r["res"] != "none":
        res_buf = torch.full((M + 1, ldres), NAN)
        res_buf[:M, :N] = res
        ref = ref + res.double()
    ref = _act64(ref, r["act"])
    idx = r["c_off"] + torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]
    return SimpleNamespace(row=r, dtype=dtype, M=M, N=N, K=K, epc=epc, a0=a0, w0=w0, lda=lda, ldw=ldw, ldc=ldc, ldres=ldres,
                           c_off=r["c_off"], c_len=r["c_off"] + (M + 1) * ldc + 8, A_buf=A_buf, W_buf=W_buf, res_buf=res_buf,
                           bias=bias if r["bias"] else None, res=r["res"], act=r["act"], out=r["out"], ref=ref, idx=idx,
                           tol=nt_tol(dtype, r))


def sentinel(n, out):
    """A flat output buffer of n elements ("f32" / "bf16") filled with the sentinel bit pattern."""
    if out == "f32":
        return torch.full((n,), SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full((n,), SENT16, dtype=torch.int16).view(torch.bfloat16)


def judge(flat, idx, ref):
    """flat: the whole output buffer back on the host (f32 or bf16, 1-D); idx: flat positions of the result's elements.
    -> (max-norm relative error of the result against ref -- NaN if an element was never written --, number of elements outside
    the result whose bits changed; counted on the int32 / int16 view)."""
    bits, sent = (flat.view(torch.int32), SENT32) if flat.dtype == torch.float32 else (flat.view(torch.int16), SENT16)
    outside = torch.ones(flat.numel(), dtype=torch.bool)
    outside[idx.reshape(-1)] = False
    touched = int((bits[outside] != sent).sum())
    return rel_err(flat[idx].float().numpy(), ref.numpy()), touched


def _strided(buf, off, rows, cols, pitch):
    """rows x cols elements at `pitch` from element `off` of buf's storage, NaN where that runs past the allocation."""
    flat = buf.reshape(-1)
    need = off + (rows - 1) * pitch + cols
    if need > flat.numel():
        flat = torch.cat([flat, torch.full((need - flat.numel(),), NAN)])
    return flat[off:].as_strided((rows, cols), (pitch, 1))


def emulate_nt(p, mistake=None):
    """What a kernel would leave in the output buffer, in the row's own arithmetic on the CPU: a plain torch float32 product of
    the operands as they sit in the padded buffers (bf16-exact, so bf16 rounding of the operands changes nothing), float32
    epilogue, the output rounded to bf16 when the row asks for that.  `mistake` restates one kernel bug:
      lda_as_K            A read at pitch K instead of lda
      drop_last_chunk     the last 16-byte chunk of K left out
      bias_partial_chunk  no bias on the columns of a partial 8-column chunk
      res_at_ldc          the residual read at pitch ldc instead of ldres
      stale_slice         the empty split-K slice contributes what an earlier launch left in the workspace (slice 0's partial)
      ldc_as_N            the result written at pitch N instead of ldc"""
    M, N, K = p.M, p.N, p.K
    A = _strided(p.A_buf, p.a0, M, K, K if mistake == "lda_as_K" else p.lda)
    W = _strided(p.W_buf, p.w0, N, K, p.ldw)
    if mistake == "drop_last_chunk":
        A, W = A[:, :K - p.epc], W[:, :K - p.epc]
    y = A @ W.T
    if mistake == "stale_slice":
        per = nt_dispatch(p.dtype, M, N, K, p.row["ws"], p.row["split"])["per"] * 8 * p.epc
        y = y + A[:, :per] @ W[:, :per].T
    if p.bias is not None:
        b = p.bias.clone()
        if mistake == "bias_partial_chunk":
            b[N // 8 * 8:] = 0
        y = y + b
    if p.res_buf is not None:
        y = y + _strided(p.res_buf, 0, M, N, p.ldc if mistake == "res_at_ldc" else p.ldres)
    y = _act64(y, p.act)
    flat = sentinel(p.c_len, p.out)
    pitch = N if mistake == "ldc_as_N" else p.ldc
    flat[p.c_off + torch.arange(M)[:, None] * pitch + torch.arange(N)[None, :]] = y.to(flat.dtype)
    return flat


def prerounding_error(p):
    """Error of the float32 result before a bf16 output rounding (the part of a bf16-output row's error the inputs decide)."""
    q = SimpleNamespace(**vars(p))
    q.out = "f32"
    return judge(emulate_nt(q), p.idx, p.ref)[0]


# ----------------------------------------------------------------------------------------------------------------------
# TN table (sq_linear_weight_grad) and the group entry
# ----------------------------------------------------------------------------------------------------------------------
def _tn(NO, NI, T, dy=0, x=0, w=0, branch="", tags=(), dy_pad="zero"):
    """dy / x / w: what lddy, ldx, lddw add to round_up(NO, 8), NI, NI (w = 1: an odd pitch, scalar epilogue)."""
    id = f"tn-NO{NO}-NI{NI}-T{T}-dy{dy}-x{x}-w{w}" + ("-nanpad" if dy_pad == "nan" else "")
    return dict(id=id, NO=NO, NI=NI, T=T, lddy=up(NO, 8) + dy, ldx=NI + x, lddw=NI + w, dy_pad=dy_pad,
                branch=branch or f"NO {NO}, NI {NI}, T {T}, lddy +{dy}, ldx +{x}, lddw +{w}",
                tags=(f"NO{NO}", f"NI{NI}", f"T{T}", f"dy+{dy}", f"x+{x}", f"w+{w}") + tuple(tags))


TN_DY_PAD_NAN = _tn(9, 72, 40, dy=8, branch="dY columns [NO, round_up(NO, 8)) hold NaN: they reach only accumulator rows that are never "
                    "stored, so a caller may leave them unspecified", tags=("dy-pad-nan",), dy_pad="nan")
TN_CASES = [
    _tn(1, 32, 40, branch="HE2RNA layers=[1]: n_out = 1 with lddy = 8", tags=("he2rna-nout1",)),
    _tn(1, 8, 1), _tn(1, 8, 2, 8, 8, 4), _tn(2, 16, 7, 0, 0, 1), _tn(2, 72, 31, 16), _tn(7, 8, 32, 0, 8, 4), _tn(7, 128, 33, 8),
    _tn(8, 16, 64), _tn(8, 136, 65, 8, 8, 1), _tn(9, 8, 333, 0, 0, 4), _tn(9, 72, 1, 16, 8), _tn(63, 16, 2), _tn(63, 128, 7, 8, 0, 1),
    _tn(65, 8, 31, 0, 8), _tn(65, 136, 32, 16, 0, 4), _tn(127, 16, 33), _tn(127, 72, 64, 8, 8, 4), _tn(128, 128, 65),
    _tn(128, 8, 333, 16, 8, 1), _tn(129, 72, 2), _tn(129, 136, 333, 8, 8, 4), _tn(1, 128, 333), _tn(2, 136, 64, 8, 0, 4),
    _tn(7, 16, 65, 16, 8, 1), _tn(8, 72, 7), _tn(9, 128, 32, 0, 0, 1), _tn(63, 136, 1, 16, 8, 4), _tn(65, 72, 33, 8),
    _tn(129, 16, 31, 0, 8, 1),
    TN_DY_PAD_NAN,
]
TN_BY_ID = {r["id"]: r for r in TN_CASES}
TN_REQUIRED_TAGS = ([f"NO{n}" for n in (1, 2, 7, 8, 9, 63, 65, 127, 128, 129)] + [f"NI{n}" for n in (8, 16, 72, 128, 136)] +
                    [f"T{t}" for t in (1, 2, 7, 31, 32, 33, 64, 65, 333)] + ["dy+0", "dy+8", "dy+16", "x+0", "x+8", "w+0", "w+4", "w+1",
                                                                               "he2rna-nout1", "dy-pad-nan"])
TN_TOL = 1e-5
DB_GUARD = 8            # sentinel floats on either side of dbias


def _group(NO, NI, T, members, ring):
    row = _tn(NO, NI, T, 8, 8, 4)
    row.update(id=f"group-NO{NO}-NI{NI}-T{T}-m{members}", members=members, dtypes=("bf16",) if ring else ("bf16", "f32"),
               branch=("ring shape: extents multiples of 128, 13 token steps; the ring form needs 8 tiles, so from two members on"
                       if ring else "not a ring shape: the two-buffer kernel, batched over the members"),
               tags=(f"members{members}", "group-ring-shape" if ring else "group-plain-shape"))
    return row


GROUP_CASES = [_group(256, 384, 777, m, True) for m in (1, 2, 3, 4)] + [_group(136, 264, 333, m, False) for m in (1, 2, 3, 4)]
GROUP_BY_ID = {r["id"]: r for r in GROUP_CASES}
GROUP_REQUIRED_TAGS = [f"members{m}" for m in (1, 2, 3, 4)] + ["group-ring-shape", "group-plain-shape"]


@functools.lru_cache(maxsize=None)
def _tn_operands(case_id, member):
    row = TN_BY_ID.get(case_id) or GROUP_BY_ID[case_id]
    NO, NI, T = row["NO"], row["NI"], row["T"]
    g = torch.Generator().manual_seed(_seed(case_id) + 17 * member)
    if NO < 64:
        dY, X = torch.rand(T, NO, generator=g) + 0.5, torch.rand(T, NI, generator=g) + 0.5
    else:
        dY = torch.randn(T, NO, generator=g) + 0.05 * member
        X = torch.randn(T, NI, generator=g) + torch.arange(NI)[None, :] * 1e-3                  # asymmetric columns
    dY, X = to_bf16_f32(dY), to_bf16_f32(X)
    return dY, X, dY.double().T @ X.double(), dY.double().sum(0)


def tn_problem(row, member=0):
    """The host side of one weight gradient (one member of a group): padded dY / X buffers, output geometry, float64 dW and
    dbias.  The same for f32 and bf16 (bf16-exact operands; lddy, ldx are multiples of 8)."""
    NO, NI, T = row["NO"], row["NI"], row["T"]
    dY, X, ref_dw, ref_db = _tn_operands(row["id"], member)
    dY_buf = torch.full((T + 1, row["lddy"]), NAN)
    dY_buf[:T, :NO] = dY
    dY_buf[:T, NO:up(NO, 8)] = NAN if row["dy_pad"] == "nan" else 0.0
    X_buf = torch.full((T + 1, row["ldx"]), NAN)
    X_buf[:T, :NI] = X
    idx = torch.arange(NO)[:, None] * row["lddw"] + torch.arange(NI)[None, :]
    return SimpleNamespace(row=row, NO=NO, NI=NI, T=T, lddy=row["lddy"], ldx=row["ldx"], lddw=row["lddw"], dY_buf=dY_buf, X_buf=X_buf,
                           dw_len=(NO + 1) * row["lddw"] + 8, db_len=NO + 2 * DB_GUARD, idx=idx, db_idx=DB_GUARD + torch.arange(NO),
                           ref_dw=ref_dw, ref_db=ref_db, tol=TN_TOL)


def emulate_tn(p, mistake=None):
    """(dW buffer, dbias buffer) a kernel would leave, plain torch float32 on the CPU.  mistake "dbias_over_lddy": the column
    sums are taken and stored for all lddy columns of dY instead of the first NO."""
    dY, X = p.dY_buf[:p.T, :p.NO], p.X_buf[:p.T, :p.NI]
    dw = sentinel(p.dw_len, "f32")
    dw[p.idx] = dY.T @ X
    db = sentinel(p.db_len, "f32")
    if mistake == "dbias_over_lddy":
        n = min(p.lddy, p.db_len - DB_GUARD)
        db[DB_GUARD:DB_GUARD + n] = p.dY_buf[:p.T].sum(0)[:n]
    else:
        db[p.db_idx] = dY.sum(0)
    return dw, db
