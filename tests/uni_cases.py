"""Case table of the UNI embedder's shape sweep, shared by tests/test_uni_cases_host.py (CPU: is the reference itself inside
the bounds at every row, and would the bounds notice a wrong attention core?) and tests/test_gpu_uni_shapes.py (GPU: the HIP
path in its three modes against the float64 oracle).

check_cfg (csrc/uni.hip) admits dim % 64 == 0 up to 4096 with heads = dim / 64, depth 1 .. SQ_UNI_MAX_DEPTH, mlp_dim % 8 == 0 and
every image size 16 .. 240 px in steps of 16 (2 .. 226 tokens, at most 256).  Every row names the branch it is there for.

Weights: oracle/uni_oracle.py's init_state_dict with LayerScale gains of O(0.5), so that both branches of every block matter.
Patches: seeded uint8.  Reference: uni_oracle.forward in float64.  Tolerances are the project's for this embedder
(test_gpu_uni.py, test_gpu_uni_x3.py): fp32 and f16x3 1e-4, bf16 5e-2, max-norm relative.  A row has to pass
test_uni_cases_host.py before it may be used on the GPU; a row that does not is replaced by another shape reaching the same
branch, never kept with a looser bound."""
import functools
from collections import OrderedDict

import numpy as np
import torch

from oracle import uni_oracle
from shape_cases import oracle_threads

TOL = {"fp32": 1e-4, "f16x3": 1e-4, "bf16": 5e-2}
# the normalised-tensor call form m(x) against extract_patches_u8 (test_gpu_uni.py, test_gpu_uni_x3.py)
TOL_DIRECT = {"fp32": 1e-6, "f16x3": 1e-6, "bf16": 2e-2}
MODES = ("fp32", "f16x3", "bf16")
# what the reference itself may use up of those bounds (float32 oracle vs float64 oracle: a tenth of the fp32 tolerance)
FLOOR_F32 = 1e-5
# a wrong attention core has to move the features by three times the fp32 bound to count as seen
TEETH = 3e-4

MAX_TOKENS = 256


def tokens(img):
    return (img // 16) ** 2 + 1


def _row(dim, heads, mlp_dim, img, depth, n, branch):
    return dict(id=f"uni-D{dim}-h{heads}-F{mlp_dim}-S{img}-L{depth}-n{n}", dim=dim, heads=heads, mlp_dim=mlp_dim, img=img, depth=depth,
                n=n, T=tokens(img), branch=branch)


# (dim, heads, mlp_dim, img, depth, n).  depth >= 2 everywhere but the last row: in the final block only the class query is read,
# so a one-block model hides every other query row.
CASES = [
    _row(128, 2, 512, 16, 2, 3, "T = 2: one patch token; the patch-embedding product has M = n"),
    _row(128, 2, 512, 64, 2, 1, "T = 17, n = 1: the reference's batch-1 call; class-row products with M = 1"),
    _row(128, 2, 512, 96, 2, 3, "T = 37: the first two-tile shape, 27 padding keys"),
    _row(128, 2, 512, 128, 2, 3, "T = 65: one key in the last tile; the fp32 kernel's lane + 64 boundary"),
    _row(192, 3, 200, 160, 2, 2, "T = 101: four tiles = exactly one pass of the 4 waves; heads not a power of two; mlp_dim 200"),
    _row(128, 2, 512, 192, 2, 2, "T = 145: five tiles, a second pass of the 4-wave query loop with one tile"),
    _row(128, 2, 512, 240, 2, 2, "T = 226: eight tiles, the largest admitted"),
    _row(1024, 16, 4096, 240, 2, 2, "the real widths (the D == 1024 vector LayerNorm) at the token limit"),
    _row(4096, 64, 64, 32, 2, 2, "widest admitted dim: generic LayerNorm with 64 values per lane; mlp_dim < dim"),
    _row(576, 9, 1000, 112, 3, 4, "dim not a multiple of 128, mlp_dim 1000, T = 50"),
    _row(64, 1, 8, 48, 1, 5, "the smallest of everything; depth 1 (the class-rows-only block is the first)"),
]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def _refusal(what, match, **over):
    cfg = dict(dim=128, heads=2, mlp_dim=512, img=64, depth=2)
    cfg.update(over)
    return dict(id=what, match=match, **cfg)


def refusals(max_depth):
    """Configurations check_cfg refuses, with a piece of the message each must fail by."""
    return [
        _refusal("img-256", "img_size=256", img=256),                     # 257 tokens
        _refusal("dim-4160", "dim=4160", dim=4160, heads=65),
        _refusal("mlp-dim-100", "mlp_dim=100", mlp_dim=100),              # not a multiple of 8
        _refusal("depth-0", "depth=0", depth=0),
        _refusal("depth-max+1", f"depth={max_depth + 1}", depth=max_depth + 1),
    ]


# the valid row that must still match after every refusal in the same process
AFTER_REFUSAL = "uni-D128-h2-F512-S96-L2-n3"


def admitted(c, max_depth):
    """check_cfg restated."""
    return (c["dim"] > 0 and c["dim"] % 64 == 0 and c["dim"] <= 4096 and c["heads"] * 64 == c["dim"] and 1 <= c["depth"] <= max_depth
            and c["mlp_dim"] > 0 and c["mlp_dim"] % 8 == 0 and c["img"] >= 16 and c["img"] % 16 == 0 and tokens(c["img"]) <= MAX_TOKENS)


def model_kwargs(c):
    """UniViT's constructor arguments for a row (or a refusal)."""
    return dict(embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"], mlp_dim=c["mlp_dim"], img_size=c["img"])


# The seeds are part of the table.  How far one wrong query row out of 226 moves the class token depends on the draw: over the
# salts 0 .. 7 the last-query mutation of test_uni_cases_host.py moved the D = 1024, T = 226 row by 2.1e-4 ... 1.1e-3 (salt 0:
# 2.1e-4, salt 3: 1.1e-3), and the D = 128, T = 226 row by 1.1e-3 at salt 0 and 1.6e-4 at salt 3.  The teeth tests need every
# row above 3e-4 with room, so that one row carries a salt -- chosen on the CPU from the oracle alone.
SEED_SALT = {"uni-D1024-h16-F4096-S240-L2-n2": 3}


def _seed(case):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) + SEED_SALT.get(case["id"], 0)) % 100003


def state_dict(case):
    return uni_oracle.init_state_dict(dim=case["dim"], depth=case["depth"], heads=case["heads"], mlp_dim=case["mlp_dim"],
                                      img_size=case["img"], seed=_seed(case), scale_ls=0.5)


def patches(case):
    """uint8 [n, S, S, 3], seeded."""
    return np.random.RandomState(_seed(case) + 1).randint(0, 256, (case["n"], case["img"], case["img"], 3), dtype=np.uint8)


def reference_uncached(case, dtype):
    """The oracle's features of the row's patches with weights and activations in `dtype`: float64 numpy [n, dim]."""
    sd = OrderedDict((k, v.to(dtype)) for k, v in state_dict(case).items())
    x = uni_oracle.transform_patch_u8(patches(case)).to(dtype)
    with oracle_threads(), torch.no_grad():
        return uni_oracle.forward(sd, x, case["heads"]).double().numpy()


@functools.lru_cache(maxsize=None)
def _reference_cached(case_id, dtype):
    out = reference_uncached(BY_ID[case_id], dtype)
    out.setflags(write=False)
    return out


def reference(case, dtype=torch.float64):
    return _reference_cached(case["id"], dtype)


# ---- deliberately wrong attention cores (q, k, v: [B, heads, N, 64]) for the teeth tests ---------------------------------

def leak_padding_key(attention):
    """One padding key inside the softmax: score 0, value 0."""
    def f(q, k, v):
        z = torch.zeros_like(k[..., :1, :])
        return attention(q, torch.cat([k, z], -2), torch.cat([v, z], -2))
    return f


def drop_last_key(attention):
    def f(q, k, v):
        return attention(q, k[..., :-1, :], v[..., :-1, :])
    return f


def last_query_from_the_row_before(attention):
    def f(q, k, v):
        o = attention(q, k, v).clone()
        o[..., -1, :] = o[..., -2, :]
        return o
    return f


MUTATIONS = OrderedDict([("padding key leaked", leak_padding_key), ("last key dropped", drop_last_key),
                         ("last query row from the row before", last_query_from_the_row_before)])
