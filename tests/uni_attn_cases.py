"""Inputs, float64 reference, error bound and checker for the UNI attention cores alone (sq_dbg_uni_attn, csrc/uni.hip), shared
by tests/test_gpu_uni_attn.py (GPU: the three kernels through the forward pass's own launch) and tests/test_uni_attn_host.py
(CPU: the checker itself on trial -- it accepts the roundings a correct kernel makes and rejects wrong cores).

Per (image, head): o = softmax(q k^T / 8) v with q, k, v [T, 64].  Three input families, every (image, head) with data of its own:

  random    q = 1.5 N(0,1); k, v = N(0,1).
  bait      q = c 1, k = -c 1 + 0.05 N(0,1) with 8 c^2 = 12: every true score is about -12, v in [1, 2].  A padding key that
            reaches the softmax with score 0 takes nearly all the weight, and its zero value the output with it.
  readback  k_j a +-1 code, q_i = 2.5 k_pi(i) for a permutation pi: the matching score is 20, the others have std 2.5;
            v[j, c] = +-(j + 1) by the parity of c.  Row i must read back pi(i) + 1: a wrong pairing of query, key or value row
            anywhere (swizzle, transposing read, lane swap, clamped query row) is a wrong integer.

All values are bf16-exact, so every mode is handed the same numbers.

The bound is per element and derived, not fitted.  With p the exact softmax weights, A = sum_j p_j |v_jc|, S = max over the
(query, key) pairs of the (image, head) of 0.125 sum_d |q_d k_d|, and u = 2^-24:

  fp32    |o - ref| <= k32 A,   k32 = 128 u S + (2 T + 8) u
          a 64-term fp32 dot product is off by at most 64 u sum|q k|; the score and the maximum it is measured from each carry
          that, so every weight is off by a relative 128 u S before the exponential's own few u; two T-term sums (the
          normaliser and P V) add 2 T u.
  f16x3   k32 + 2^-19: three operands (P, V, the output) each as hi + lo fp16 planes good to 2^-22 of the value, with the
          three-term products dropping lo.lo (another 2^-22 per product).
  bf16    k32 + 2^-7: P rounded to bf16 (2^-8 relative per weight) and the output rounded to bf16 (2^-8).
"""
import functools
from collections import OrderedDict

import torch

N_IMG, HEADS, DH = 2, 3, 64
FAMILIES = ("random", "bait", "readback")
MODES = ("fp32", "f16x3", "bf16")
# the token counts of the 15 admitted image sizes (16 .. 240 px), and the edges of the 32-key tiles no image size produces
PRODUCTION_T = tuple((g * g + 1) for g in range(1, 16))
EDGE_T = (1, 31, 32, 33, 64, 255, 256)
ALL_T = tuple(sorted(set(PRODUCTION_T) | set(EDGE_T)))
U = 2.0 ** -24
EXTRA = {"fp32": 0.0, "f16x3": 2.0 ** -19, "bf16": 2.0 ** -7}


def _bf16_exact(t):
    return t.to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def inputs(family, T):
    """dict(q, k, v: float64 [N_IMG, HEADS, T, 64], bf16-exact; perm: int64 [N_IMG, HEADS, T] for readback)."""
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + T)
    shape = (N_IMG, HEADS, T, DH)
    out = {}
    if family == "random":
        q, k, v = 1.5 * torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    elif family == "bait":
        c = 1.5 ** 0.5
        q = torch.full(shape, c)
        k = -c + 0.05 * torch.randn(shape, generator=g)
        v = 1.0 + torch.rand(shape, generator=g)
    else:
        k = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        perm = torch.stack([torch.randperm(T, generator=g) for _ in range(N_IMG * HEADS)]).view(N_IMG, HEADS, T)
        q = 2.5 * torch.gather(k, 2, perm[..., None].expand(shape))
        sign = 1.0 - 2.0 * (torch.arange(DH) % 2)
        v = (torch.arange(T) + 1.0)[:, None] * sign[None, :] * torch.ones(N_IMG, HEADS, 1, 1)
        out["perm"] = perm
    out.update(q=_bf16_exact(q), k=_bf16_exact(k), v=_bf16_exact(v))
    return out


def attention64(q, k, v):
    """The reference: softmax(q k^T / 8) v in float64."""
    p = (0.125 * (q @ k.transpose(-2, -1))).softmax(-1)
    return p @ v


def bound_terms(q, k, v):
    """(ref, A, k32) in float64: ref and A [n, H, T, 64], k32 [n, H, 1, 1]."""
    T = q.shape[-2]
    p = (0.125 * (q @ k.transpose(-2, -1))).softmax(-1)
    S = (0.125 * (q.abs() @ k.abs().transpose(-2, -1))).amax(dim=(-2, -1), keepdim=True)
    return p @ v, p @ v.abs(), 128 * U * S + (2 * T + 8) * U


def verdict(mode, got, q, k, v, perm=None):
    """(ok, ratio): ratio = max |got - ref| / (kappa A) over the elements; ok = ratio <= 1, every element finite, and -- with
    `perm` -- every row of got within 0.5 of the integer pi(i) + 1 it has to read back."""
    ref, A, k32 = bound_terms(q, k, v)
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return False, float("inf")
    ratio = float(((got - ref).abs() / ((k32 + EXTRA[mode]) * A)).max())
    ok = ratio <= 1.0
    if perm is not None:
        ok = ok and bool(((got.abs() - (perm[..., None] + 1.0)).abs() < 0.5).all())
    return ok, ratio


# ---- layouts of the forward pass -----------------------------------------------------------------------------------------

def pack_qkv(q, k, v):
    """[n, H, T, 64] x 3 -> [n T, 3 H 64]: columns (q | k | v), each H blocks of 64."""
    n, H, T, _ = q.shape
    return torch.cat([t.permute(0, 2, 1, 3).reshape(n * T, H * DH) for t in (q, k, v)], 1).contiguous()


def unpack_o(o, n, H, T):
    """[n T, H 64] -> [n, H, T, 64]."""
    return o.reshape(n, T, H, DH).permute(0, 2, 1, 3)


def unpack_qkv(qkv, n, H, T):
    return tuple(unpack_o(qkv[:, i * H * DH:(i + 1) * H * DH], n, H, T) for i in range(3))


# ---- what a correct kernel may do: the roundings of the bf16 core, and plain float32 -----------------------------------------

def emulate_bf16_core(q, k, v):
    """The rounding points of uni_attn_mfma_kernel on the CPU: fp32 unscaled scores, 2^x of one fma, P rounded to bf16, fp32 P V,
    division by the sum of the unrounded weights, the output rounded to bf16."""
    q, k, v = q.float(), k.float(), v.float()
    s = q @ k.transpose(-2, -1)
    cexp = torch.tensor(0.125 * 1.44269504088896340736, dtype=torch.float32)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp2(torch.addcmul(-mx * cexp, s, cexp))
    o = (e.to(torch.bfloat16).float() @ v) * (1.0 / e.sum(-1, keepdim=True))
    return o.to(torch.bfloat16).double()


def float32_core(q, k, v):
    return attention64(q.float(), k.float(), v.float()).double()


# ---- wrong cores the checker has to reject -------------------------------------------------------------------------------

def _leak(q, k, v):
    z = torch.zeros_like(k[..., :1, :])
    return attention64(q, torch.cat([k, z], -2), torch.cat([v, z], -2))


def _drop(q, k, v):
    return attention64(q, k[..., :-1, :], v[..., :-1, :])


def _last_query(q, k, v):
    o = attention64(q, k, v).clone()
    o[..., -1, :] = o[..., -2, :]
    return o


def _swap_v(q, k, v):
    v = v.clone()
    v[..., [0, -1], :] = v[..., [-1, 0], :]
    return attention64(q, k, v)


def _swap_heads(q, k, v):
    return attention64(q, k, v)[:, [1, 0, 2]]


def _swap_images(q, k, v):
    return attention64(q, k, v)[[1, 0]]


MUTANTS = OrderedDict([("one zero key leaked", _leak), ("last key dropped", _drop), ("last query row copied from the one before", _last_query),
                       ("two V rows swapped", _swap_v), ("heads swapped", _swap_heads), ("images swapped", _swap_images)])
