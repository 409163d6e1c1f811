"""Bit-parity fixture of the HE2RNA comparator: what the model computed BEFORE its parameters moved into one flat buffer.
    python tests/golden/make_he2rna_parity.py parity   -> tests/golden/he2rna_flat_parity.npz      (on the MI355X)
    python tests/golden/make_he2rna_parity.py pickle   -> tests/golden/he2rna_parent_module.{pt,npz} (on the CPU)
Both were run once, at the commit in front of the flat-parameter refactor (the module then owned ``nn.Conv1d`` containers; its
whole-module pickle has ``conv{i}`` submodules and no ``flat``).  `record` is also what tests/test_gpu_he2rna_parity.py runs on
the current code: `_grads` is the one place that knows both forms.

Three stacks on B = 3 slides of N = 20 tiles with C = 35 channels, G = 12 genes, ks = [1, 5, 20]: layers=[1] on the last 32
channels (a hidden width of ONE), layers=[5, 12] on the last 30 (no width a multiple of 8), layers=[16, 16] on the last 32 (every
width a multiple of 8).  Seeded weights and inputs; tiles are masked (all channels <= 0) in the middle and at the end of a slide,
never at its start (no 0/0).  Per stack (`record`):
  eval, fixed_k5, conv, tile_scores ([:, :G]), tile_mask, window_predictions       the forward forms, eval mode
  grad_eval/<key>, grad_fixed_k5/<key>, .../x                                      gradients of (pred * r).sum()
  train_loss, train_grad/<key>     torch.manual_seed(21); np.random.seed(21), dropout 0.5, training mode, the first batch's MSE
                                   loss and gradients: the order in which the autograd path consumes the two RNG streams
  fused_losses, fused_final/<key>  He2rnaTrainStep(lr 3e-3, seed=1234), dropout 0.5, np.random.seed(21): three steps"""
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd.he2rna import HE2RNA, He2rnaTrainStep  # noqa: E402

KS, LR = [1, 5, 20], 3e-3
B, C, N, G = 3, 35, 20, 12
STACKS = {
    "layers1": dict(layers=[1], D=32, seed=31),
    "layers5x12": dict(layers=[5, 12], D=30, seed=32),
    "layers16x16": dict(layers=[16, 16], D=32, seed=33),
}
DEV = "cuda:0"


def _grads(m):
    """Per-tensor gradients under the state_dict keys: slices of the flat gradient, or (before the refactor) the containers'."""
    if hasattr(m, "flat"):
        return m.grad_views(m.flat.grad)
    return {k: p.grad for k, p in m.named_parameters()}


def inputs(name):
    """(state dict, x f32 [B, C, N], loss weights r f32 [B, G], targets y f32 [B, G]) of one stack, on the CPU."""
    c = STACKS[name]
    g = torch.Generator().manual_seed(c["seed"])
    dims = [c["D"]] + c["layers"] + [G]
    sd = {}
    for i in range(len(dims) - 1):
        sd[f"conv{i}.weight"] = (torch.rand(dims[i + 1], dims[i], 1, generator=g) - 0.35) / dims[i] ** 0.5
        sd[f"conv{i}.bias"] = torch.rand(dims[i + 1], generator=g) * 0.2 - 0.05
    x = torch.randn(B, C, N, generator=g).clamp_min(-0.2)
    x[0, :, 7] = 0
    x[0, :, 19] = -0.1
    x[1, :, 10:12] = 0
    x[2, :, 17:] = 0
    return sd, x, torch.randn(B, G, generator=g), torch.rand(B, G, generator=g) * 3


def model(name, device=DEV):
    c = STACKS[name]
    m = HE2RNA(input_dim=c["D"], output_dim=G, layers=c["layers"], ks=KS, dropout=0.5, device=device)
    m.load_state_dict(inputs(name)[0])
    return m


def fused_steps(m, name, steps):
    """`steps` fused training steps on the stack's batch; returns the losses (device tensor [steps])."""
    _, x, _, y = inputs(name)
    np.random.seed(21)
    tr = He2rnaTrainStep(m.train(), LR, seed=1234)
    xb = x.transpose(1, 2).contiguous()                                  # as the loader gives it: tiles x channels
    return torch.stack([tr.step(xb, y) for _ in range(steps)])


def record(name):
    """Everything the fixture holds for one stack, as numpy arrays, computed on cuda:0."""
    sd, x, r, y = inputs(name)
    xd, rd = x.to(DEV), r.to(DEV)
    out = {}
    m = model(name).eval()
    with torch.no_grad():
        out["eval"], out["fixed_k5"], out["conv"] = m(xd), m.forward_fixed_k(xd, 5), m.conv(xd)
        scores, mask = m.tile_scores(xd.transpose(1, 2).reshape(B * N, C).contiguous())
        members = torch.arange(B * N, dtype=torch.int32, device=DEV).view(B, N).clone()
        members[2, 17:] = -1                                             # zero padding behind the tiles of the last window
        out["tile_scores"], out["tile_mask"] = scores[:, :G], mask
        out["window_predictions"] = m.window_predictions(scores, mask, members)
    for form in ("eval", "fixed_k5"):
        m.zero_grad()
        xg = xd.clone().requires_grad_(True)
        pred = m(xg) if form == "eval" else m.forward_fixed_k(xg, 5)
        (pred * rd).sum().backward()
        out.update({f"grad_{form}/{k}": g.clone() for k, g in _grads(m).items()})
        out[f"grad_{form}/x"] = xg.grad
    torch.manual_seed(21)
    np.random.seed(21)
    m.train()
    m.zero_grad()
    loss = torch.nn.functional.mse_loss(m(xd), y.to(DEV))
    loss.backward()
    out["train_loss"] = loss
    out.update({f"train_grad/{k}": g.clone() for k, g in _grads(m).items()})
    m2 = model(name)
    out["fused_losses"] = fused_steps(m2, name, 3)
    out.update({f"fused_final/{k}": v for k, v in m2.state_dict().items()})
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in out.items()}


def main(what, out=None):
    if what == "parity":
        arrays = {f"{name}/{k}": v for name in STACKS for k, v in record(name).items()}
        np.savez(out or os.path.join(GOLDEN, "he2rna_flat_parity.npz"), **arrays)
    elif what == "pickle":                                                # a whole-module pickle as fit() writes model[_fold].pt
        if hasattr(HE2RNA, "padding_mask"):
            raise SystemExit("this class already keeps its parameters in `flat`: only the commit in front of it can write the old form")
        torch.manual_seed(5)
        m = HE2RNA(input_dim=30, output_dim=7, layers=[5, 12], ks=[1, 5], dropout=0.25, device="cpu")
        torch.save(m, os.path.join(GOLDEN, "he2rna_parent_module.pt"))
        np.savez(os.path.join(GOLDEN, "he2rna_parent_module.npz"), **{k: v.numpy() for k, v in m.state_dict().items()})
    else:
        raise SystemExit("usage: make_he2rna_parity.py parity|pickle [out.npz]")


if __name__ == "__main__":
    main(*sys.argv[1:3])
