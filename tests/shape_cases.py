"""Case table of the ViS / ViT shape sweep, shared by tests/test_oracle_shape_floor.py (CPU: is the reference itself
inside the bounds at every row?) and tests/test_gpu_shape_contract.py (GPU: the HIP path against the float64 oracle).

Every row names the launch-code branch it is there for.  The reference of every assertion is oracle/vis_oracle.py +
autograd run in float64 on seeded synthetic weights with non-trivial LayerNorm gains and biases.

Tolerances are the project's (BASELINE north_star; test_gpu_vis.py, test_gpu_train.py, test_gpu_vit.py): fp32 mode 1e-4 for
predictions, loss and every gradient tensor; bf16 mode predictions 3e-2, gradient tensors 8e-2, loss 2e-2 relative.  A row
has to pass test_oracle_shape_floor.py before it may be used on the GPU; a row that does not is replaced by another shape
reaching the same branch, never kept with a looser bound."""
import contextlib
import functools
from collections import OrderedDict

import torch
import torch.nn.functional as F

from gpu_util import rel_err
from oracle import vis_oracle

TOL = {"fp32": dict(pred=1e-4, loss=1e-4, grad=1e-4), "bf16": dict(pred=3e-2, loss=2e-2, grad=8e-2)}
# what the reference itself may use up of those bounds (float32 oracle vs float64 oracle: a tenth of the fp32 tolerance)
FLOOR_F32 = 1e-5


def _vis(D, nheads, depth, N, B, G, branch, backward="ok", **kw):
    return dict(kind="vis", id=f"vis-D{D}-h{nheads}-L{depth}-N{N}-B{B}-G{G}", D=D, nheads=nheads, depth=depth, N=N, B=B, G=G,
                branch=branch, backward=backward, **kw)


def _vit(dim, heads, mlp_dim, N, depth, B, G, branch, backward="ok", **kw):
    return dict(kind="vit", id=f"vit-D{dim}-h{heads}-F{mlp_dim}-N{N}-L{depth}-B{B}-G{G}", D=dim, heads=heads, mlp_dim=mlp_dim,
                N=N, depth=depth, B=B, G=G, branch=branch, backward=backward, **kw)


POW2 = "power of two"          # sq_vis_backward's refusal
LDS = "LDS"                    # sq_vit_backward's refusal

# (D, nheads, depth, N, B, G)
VIS_CASES = [
    _vis(4096, 2, 1, 16, 3, 96, "ln_rows<16> forward / backward, lean <8>"),
    _vis(3072, 64, 1, 24, 2, 72, "ln64_gelu_bwd NCH=4, lean rpi_l=1, D > 2048 with the widest head block"),
    _vis(1536, 32, 2, 40, 3, 50, "ln_rows<8,bf16-in>, ln_rows_bwd<8> / lean <4>, ln64_gelu_bwd NCH=2"),
    _vis(2048, 8, 2, 100, 2, 120, "the headline's input_dim with a backward pass; nheads 8"),
    _vis(64, 1, 1, 1, 1, 8, "N = 1 and M = 1: one token row in every weight gradient"),
    _vis(64, 1, 1, 1, 4, 8, "N = 1, four slides"),
    _vis(128, 2, 2, 300, 3, 40, "N above the tile height (row bias / group sums)"),
    _vis(128, 2, 2, 128, 3, 40, "N equal to the tile height"),
    _vis(128, 2, 2, 7, 9, 40, "many slides per tile, ragged"),
    _vis(128, 2, 1, 8, 520, 24, "B > 512: column sums on the helper stream instead of the deferred launch"),
    _vis(192, 3, 2, 100, 5, 72, "nheads not a power of two: forward only, backward refused", backward=POW2),
    _vis(320, 5, 1, 129, 2, 33, "nheads not a power of two, N = 129: forward only, backward refused", backward=POW2),
]

# bf16 inference with the combiner in the f projection's epilogue (vis.hip: bf16, no save, HD % 256 == 0, M >= 65 536 and the
# 256 x 256 eight-phase GEMM: K = D >= 512, at least 176 tiles): M = 70 000 = 273 tiles + a ragged one; oracle on the first slides
VIS_FUSED_COMBINER = _vis(512, 4, 2, 50, 1400, 1000, "combiner in the gemm_p8 epilogue off N = 100", backward="none", oracle_slides=6)

# (dim, heads, mlp_dim, N, depth, B, G)
VIT_CASES = [
    _vit(128, 3, 192, 100, 2, 3, 40, "heads*64 != dim, mlp_dim != 2*dim"),
    _vit(256, 1, 64, 1, 1, 4, 8, "one key"),
    _vit(128, 2, 256, 63, 2, 3, 40, "lane + 64 boundary: N = 63"),
    _vit(128, 2, 256, 64, 2, 3, 40, "lane + 64 boundary: N = 64"),
    _vit(128, 2, 256, 65, 2, 3, 40, "lane + 64 boundary: N = 65"),
    _vit(192, 2, 320, 111, 2, 2, 24, "the largest N with a backward pass"),
    _vit(192, 2, 320, 112, 2, 2, 24, "the smallest N the backward pass refuses", backward=LDS),
    _vit(1536, 4, 2048, 128, 1, 2, 24, "forward at the N limit; backward refused", backward=LDS),
    _vit(4096, 2, 64, 16, 1, 3, 48, "ln_rows<16> through the ViT's fp32-stream calls"),
    _vit(1024, 16, 2048, 100, 2, 3, 500, "--model_type vit's real shape with its backward pass"),
]

ALL_CASES = VIS_CASES + [VIS_FUSED_COMBINER] + VIT_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)

# sliding-window (gather) form: case id -> rows in the tile-feature cache
GATHER_CASES = [("vis-D128-h2-L2-N7-B9-G40", 41), ("vis-D2048-h8-L2-N100-B2-G120", 150), ("vit-D128-h2-F256-N65-L2-B3-G40", 90)]

# a small valid step run after every refusal: the refused call must leave the process usable
VIS_AFTER_REFUSAL = "vis-D128-h2-L2-N7-B9-G40"
VIT_AFTER_REFUSAL = "vit-D128-h2-F256-N65-L2-B3-G40"


ORACLE_THREADS = 16


@contextlib.contextmanager
def oracle_threads():
    """The oracle's CPU arithmetic runs on exactly 16 threads, whatever the machine's core count (never sized from
    os.cpu_count()).  Exactly, not at most: torch's CPU LayerNorm backward in bfloat16 keeps one partial sum of the gain / bias gradients per
    thread IN bfloat16, so the bfloat16 oracle's error on those tensors depends on the thread count where a LayerNorm sees
    thousands of rows -- at the B = 520 row (4160 rows) the FeedForward LayerNorm's bias gradient is 8.3e-1 / 6.6e-1 / 3.8e-1 /
    1.7e-1 / 3.5e-2 off the float64 oracle with 1 / 2 / 4 / 8 / 16 threads.  The float64 and float32 oracles do not depend on it."""
    n = torch.get_num_threads()
    torch.set_num_threads(ORACLE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) % 100003


def state_dict(case):
    s = _seed(case)
    if case["kind"] == "vis":
        sd = vis_oracle.init_vis_state_dict(num_outputs=case["G"], input_dim=case["D"], depth=case["depth"], nheads=case["nheads"],
                                            dimensions_f=64, dimensions_s=64, dimensions_c=64, num_clusters=case["N"], seed=s)
    else:
        sd = vis_oracle.init_vit_state_dict(num_outputs=case["G"], dim=case["D"], depth=case["depth"], heads=case["heads"],
                                            mlp_dim=case["mlp_dim"], num_clusters=case["N"], seed=s)
    return vis_oracle.perturb_norm_params(sd, seed=s + 1)


def inputs(case):
    """x f32 [B, N, D] tokens, y f32 [B, G] targets (the range of log-expression targets)."""
    g = torch.Generator().manual_seed(_seed(case) + 2)
    x = torch.randn(case["B"], case["N"], case["D"], generator=g)
    y = torch.rand(case["B"], case["G"], generator=g) * 8
    return x, y


def gather_inputs(case, rows):
    """cache f32 [rows, D], members int32 [B, N] with every index inside the cache and about one in eight -1 (a zero row)."""
    g = torch.Generator().manual_seed(_seed(case) + 3)
    cache = torch.randn(rows, case["D"], generator=g)
    members = torch.randint(0, rows, (case["B"], case["N"]), generator=g, dtype=torch.int32)
    pad = torch.rand(case["B"], case["N"], generator=g) < 0.125
    members[pad] = -1
    members[0, 0] = -1
    assert int(members.max()) < rows and int(members.min()) >= -1
    return cache, members


def gathered_tokens(cache, members):
    idx = members.long().clamp(min=0)
    x = cache[idx]
    x[members < 0] = 0
    return x


def forward(case, sd, x):
    if case["kind"] == "vis":
        return vis_oracle.vis_forward(sd, x)
    return vis_oracle.vit_forward(sd, x, case["heads"])


def reference_uncached(case, dtype, forward_only=False):
    """Oracle forward (+ MSE + autograd) with state dict, input and target in `dtype`.  Returns float64 numpy arrays:
    dict(pred, loss, grads {key: array}, gx)."""
    with oracle_threads():
        return _reference(case, dtype, forward_only)


def _reference(case, dtype, forward_only):
    sd = OrderedDict((k, v.to(dtype)) for k, v in state_dict(case).items())
    x, y = inputs(case)
    n = case.get("oracle_slides")
    if n:
        x, y = x[:n], y[:n]
    x, y = x.to(dtype), y.to(dtype)
    if forward_only or case["backward"] == "none":
        with torch.no_grad():
            return dict(pred=forward(case, sd, x).double().numpy())
    leaf = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in sd.items())
    xl = x.clone().requires_grad_(True)
    pred = forward(case, leaf, xl)
    loss = F.mse_loss(pred, y)
    loss.backward()
    return dict(pred=pred.detach().double().numpy(), loss=float(loss.detach().double()),
                grads=OrderedDict((k, v.grad.double().numpy()) for k, v in leaf.items()), gx=xl.grad.double().numpy())


@functools.lru_cache(maxsize=None)
def _reference_cached(case_id, dtype):
    return reference_uncached(BY_ID[case_id], dtype)


def reference(case, dtype=torch.float64):
    return _reference_cached(case["id"], dtype)


def gather_reference(case, rows, dtype=torch.float64):
    sd = OrderedDict((k, v.to(dtype)) for k, v in state_dict(case).items())
    cache, members = gather_inputs(case, rows)
    with oracle_threads(), torch.no_grad():
        return forward(case, sd, gathered_tokens(cache, members).to(dtype)).double().numpy()


def error_table(got, ref):
    """Per-tensor max-norm relative errors of one step against the reference: dict(pred, loss, gx, grads {key: err})."""
    out = dict(pred=rel_err(got["pred"], ref["pred"]))
    if "loss" in got:
        out["loss"] = abs(got["loss"] - ref["loss"]) / abs(ref["loss"])
        out["gx"] = rel_err(got["gx"], ref["gx"])
        out["grads"] = OrderedDict((k, rel_err(got["grads"][k], v)) for k, v in ref["grads"].items())
    return out


def worst_grad(table):
    k = max(table["grads"], key=lambda k: table["grads"][k])
    return k, table["grads"][k]
