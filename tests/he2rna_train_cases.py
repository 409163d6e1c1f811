"""Shared by tests/test_he2rna_train_host.py and tests/test_gpu_he2rna_train.py: the seeded configurations of the HE2RNA
training-step tests and their float64 reference -- autograd over oracle/he2rna_oracle.py plus a restated Adam.  Not a test
module.  Everything here runs on the CPU; references are computed once per configuration and never modified."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import he2rna_oracle as ho  # noqa: E402

ALL_KS = [1, 2, 5, 10, 20, 50, 100]
CONFIGS = {
    # hidden width ONE (the reference's default), 35 channels of which the last 32 go in
    "l1": dict(layers=[1], D=32, C=35, B=3, N=20, G=12, ks=[1, 5, 20], seed=21),
    # no width and no input_dim a multiple of 8 (nor of 4: the scalar tails)
    "l5x12": dict(layers=[5, 12], D=30, C=35, B=3, N=20, G=12, ks=[1, 5, 20], seed=22),
    # more than one block of genes (203 > 128), 100 tiles, the experiment's seven ks
    "mid": dict(layers=[24, 40], D=64, C=64, B=5, N=100, G=203, ks=ALL_KS, seed=23),
}
STEPS, LR, K_SEED = 12, 3e-3, 5


def up8(n):
    return (n + 7) // 8 * 8


def param_layout(dims):
    """The flat padded layout restated: layer i's weight [dims[i + 1], round_up(dims[i], 8)] row-major, then its bias; every
    tensor starts on a 16-byte boundary (a multiple of 4 floats).  Returns (weight offsets, bias offsets, total) in floats."""
    w_off, b_off, off = [], [], 0
    for n_in, n_out in zip(dims[:-1], dims[1:]):
        off = (off + 3) // 4 * 4
        w_off.append(off)
        off += n_out * up8(n_in)
        off = (off + 3) // 4 * 4
        b_off.append(off)
        off += n_out
    return w_off, b_off, (off + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def case(name):
    """(config, state dict f32, three batches [(x f32 [B, N, C], y f32 [B, G])]).  x = randn.clamp_min(-0.2); tiles are masked
    (all channels <= 0) in the middle and at the end of a slide, never at its start (no 0/0); y = rand * 3."""
    c = CONFIGS[name]
    g = torch.Generator().manual_seed(c["seed"])
    dims = [c["D"]] + c["layers"] + [c["G"]]
    sd = {}
    for i in range(len(dims) - 1):
        sd[f"conv{i}.weight"] = (torch.rand(dims[i + 1], dims[i], 1, generator=g) - 0.35) / dims[i] ** 0.5
        sd[f"conv{i}.bias"] = torch.rand(dims[i + 1], generator=g) * 0.2 - 0.05
    batches = []
    for _ in range(3):
        x = torch.randn(c["B"], c["N"], c["C"], generator=g).clamp_min(-0.2)
        x[0, 7] = 0
        x[0, c["N"] - 1] = -0.1
        x[1, 10:12] = 0
        x[2, c["N"] - 3:] = 0
        assert bool((x[:, 0].max(dim=1)[0] > 0).all())
        batches.append((x, torch.rand(c["B"], c["G"], generator=g) * 3))
    return c, sd, batches


def forward_k(sd, x_bnc, k, D, gates=None):
    """forward_fixed_k of the oracle for x as the loader gives it, [B, N, C].  `gates` (one [B * N, width] factor table per hidden
    layer) replaces ReLU and dropout of that layer by a multiplication -- the replay of a step whose saved activation a gives
    the gate (a > 0) / (1 - p); without gates this IS oracle.forward_fixed_k."""
    x = x_bnc.transpose(1, 2)                                       # 'b c f -> b f c': channels x tiles
    if gates is None:
        return ho.forward_fixed_k(sd, x, k, D)
    B, C, N = x.shape
    n_layers = len(sd) // 2
    h = x[:, C - D:]
    for i in range(n_layers):
        h = F.conv1d(h, sd[f"conv{i}.weight"], sd[f"conv{i}.bias"])
        if i + 1 < n_layers:
            h = h * gates[i].view(B, N, -1).transpose(1, 2)
    mask = ho.tile_mask(x)
    t, _ = torch.topk(h * mask, k, dim=2, largest=True, sorted=True)
    return torch.sum(t * mask[:, :, :k], dim=2) / torch.sum(mask[:, :, :k], dim=2)


def replay_gate(a, p):
    """The factor a step applied to a hidden unit, from its saved post-dropout activation alone: 1 / (1 - p) where a > 0, else 0."""
    return (a > 0).to(torch.float64) / (1.0 - p)


def loss_and_grads(sd, x, y, k, D, gates=None):
    """float64 MSE loss and gradients per state-dict key, by autograd through the oracle."""
    leaf = {n: v.detach().double().requires_grad_(True) for n, v in sd.items()}
    loss = F.mse_loss(forward_k(leaf, x.double(), k, D, gates), y.double())
    loss.backward()
    return float(loss.detach()), {n: v.grad for n, v in leaf.items()}


def adam_update(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam(lr, weight_decay=0.) restated, in place on float64 tensors; t is the 1-based step count."""
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = (v.sqrt() / (1 - b2 ** t) ** 0.5).add_(eps)
    p.addcdiv_(m, denom, value=-lr / (1 - b1 ** t))


def trajectory(sd, batches, ks, D, steps=STEPS, lr=LR, k_seed=K_SEED):
    """`steps` Adam steps in float64, batches cycled, the k of a step drawn as ``RandomState(k_seed).choice(ks)`` (the stream
    ``np.random.seed(k_seed); np.random.choice(ks)`` gives).  Returns (losses, final parameters, gradients of step 1)."""
    rs = np.random.RandomState(k_seed)
    p = {n: v.detach().double().clone() for n, v in sd.items()}
    m = {n: torch.zeros_like(v) for n, v in p.items()}
    v2 = {n: torch.zeros_like(v) for n, v in p.items()}
    losses, first = [], None
    for t in range(1, steps + 1):
        x, y = batches[(t - 1) % len(batches)]
        loss, grads = loss_and_grads(p, x, y, int(rs.choice(np.array(ks))), D)
        first = first or {n: g.clone() for n, g in grads.items()}
        losses.append(loss)
        for n in p:
            adam_update(p[n], grads[n], m[n], v2[n], t, lr)
    return losses, p, first


@functools.lru_cache(maxsize=None)
def reference_trajectory(name):
    c, sd, batches = case(name)
    return trajectory(sd, batches, c["ks"], c["D"])
