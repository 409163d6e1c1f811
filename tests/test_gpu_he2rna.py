"""HE2RNA comparator on the HIP engine (sequoia_pub_amd/he2rna.py) against the golden vectors of the reference's own
class (tests/golden/he2rna.npz) and, at the size pretrain_gtex.py builds it, against the pinned oracle."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sequoia_pub_amd  # noqa: E402,F401
from sequoia_pub_amd import _lib  # noqa: E402
from sequoia_pub_amd.he2rna import HE2RNA, fit  # noqa: E402
from oracle import he2rna_oracle as ho  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "he2rna.npz")


def _golden_model():
    d = np.load(GOLD)
    sd = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w_")}
    D, G = sd["conv0.weight"].shape[1], sd["conv2.weight"].shape[0]
    m = HE2RNA(input_dim=D, output_dim=G, layers=[16, 16], ks=list(d["ks"]), dropout=0.5, device="cuda:0")
    m.load_state_dict(sd)
    return d, m, torch.from_numpy(d["x"]).cuda()


def test_forward_matches_reference_golden():
    _lib.require_gpu()
    d, m, x = _golden_model()
    m.eval()
    with torch.no_grad():
        ev = m(x).cpu().numpy()
    assert np.array_equal(np.isnan(ev), np.isnan(d["pred_eval"])) and np.isnan(ev[3]).all()      # 0/0 quirk reproduced
    np.testing.assert_allclose(ev[:3], d["pred_eval"][:3], rtol=1e-4, atol=1e-5)                 # north_star: 1e-4 relative, fp32
    for k in (1, 10, 100):
        with torch.no_grad():
            got = m.forward_fixed_k(x, k).cpu().numpy()
        ref = d["fixed_%d" % k]
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(ref), rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        sc = m.conv(x).cpu()                                                                   # [B, G, N] like the reference's conv()
    ref_sc = ho.scores({k: v.cpu() for k, v in m.state_dict().items()}, x.cpu(), m.input_dim)
    np.testing.assert_allclose(sc.numpy(), ref_sc.numpy(), rtol=1e-4, atol=1e-5)


def test_gradients_match_reference_golden():
    _lib.require_gpu()
    d, m, x = _golden_model()
    m.eval()                                                   # dropout off, as in the golden run
    xg = x.clone().requires_grad_(True)
    (m.forward_fixed_k(xg, 20) * torch.from_numpy(d["r"]).cuda()).sum().backward()
    for name, g in m.grad_views(m.flat.grad).items():
        ref = d["g_" + name]
        assert g.shape == ref.shape
        np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    np.testing.assert_allclose(xg.grad.cpu().numpy(), d["grad_x"], rtol=1e-4, atol=1e-4 * np.abs(d["grad_x"]).max())


@pytest.mark.parametrize("layers", [[16, 16], [1]], ids=["hidden16x16", "hidden_width_one"])
def test_the_three_users_of_the_layer_stack_agree_bit_for_bit(layers):
    """conv() (the inspection helper), tile_scores() (the sliding-window score table) and forward() run the same layer stack on
    the same rows: in eval mode their bits are equal.  35 channels > input_dim 32: the channel slice of he2rna.py:102;
    layers=[1]: a hidden width of one, zero-padded to 8 columns; M = 2 * 20 = 40 rows: one launch on every path."""
    _lib.require_gpu()
    torch.manual_seed(6)
    D, G, B, C, N = 32, 12, 2, 35, 20
    m = HE2RNA(input_dim=D, output_dim=G, layers=layers, ks=[1, 5, 20], dropout=0.5, device="cuda:0").eval()
    x = torch.randn(B, C, N, generator=torch.Generator().manual_seed(7)).clamp_min(-0.2).cuda()
    cache = x.transpose(1, 2).reshape(B * N, C).contiguous()         # one tile per row, as the spatial path holds them
    with torch.no_grad():
        per_tile = m.conv(x).transpose(1, 2).reshape(B * N, G)       # [B, G, N] -> [B * N, G]
        scores, mask = m.tile_scores(cache)
        assert torch.equal(per_tile, scores[:, :G])
        members = torch.arange(B * N, dtype=torch.int32, device="cuda:0").view(B, N)
        pred = m(x)
        assert pred.shape == (B, G) and bool(torch.isfinite(pred).all())
        assert torch.equal(pred, m.window_predictions(scores, mask, members))


NARROW_KS = [1, 5, 20]
NARROW_STACKS = {      # B = 3 slides of N = 20 tiles with C = 35 channels, G = 12 genes
    "layers1": dict(layers=[1], D=32, seed=11),                   # the reference's default: a hidden width of ONE
    "layers5x12": dict(layers=[5, 12], D=30, seed=12),            # no width and no input_dim a multiple of 8
}


@functools.lru_cache(maxsize=None)
def _narrow_stack(name):
    """Seeded state dict, input and loss weights of one stack, and the float64 reference (oracle + autograd) of both forward
    forms: dict(pred, grads {key: array}, gx) per form.  Tiles are masked (all channels <= 0) in the middle and at the end of a
    slide, never at its start (no 0/0).  Computed once, shared by the cases, never modified."""
    c = NARROW_STACKS[name]
    B, C, N, G, D = 3, 35, 20, 12, c["D"]
    g = torch.Generator().manual_seed(c["seed"])
    dims = [D] + c["layers"] + [G]
    sd = {}
    for i in range(len(dims) - 1):
        sd[f"conv{i}.weight"] = (torch.rand(dims[i + 1], dims[i], 1, generator=g) - 0.35) / dims[i] ** 0.5
        sd[f"conv{i}.bias"] = torch.rand(dims[i + 1], generator=g) * 0.2 - 0.05
    x = torch.randn(B, C, N, generator=g).clamp_min(-0.2)
    x[0, :, 7] = 0
    x[0, :, 19] = -0.1
    x[1, :, 10:12] = 0
    x[2, :, 17:] = 0
    r = torch.randn(B, G, generator=g)
    refs = {}
    for form in ("fixed_k5", "eval_mean"):
        leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        xl = x.double().requires_grad_(True)
        pred = ho.forward_fixed_k(leaf, xl, 5, D) if form == "fixed_k5" else ho.forward_eval(leaf, xl, NARROW_KS, D)
        (pred * r.double()).sum().backward()
        refs[form] = dict(pred=pred.detach().numpy(), grads={k: v.grad.numpy() for k, v in leaf.items()}, gx=xl.grad.numpy())
    hidden = torch.nn.functional.conv1d(x[:, C - D:].double(), sd["conv0.weight"].double(), sd["conv0.bias"].double())     # [B, width, N]
    return sd, x, r, refs, (hidden > 0)


@pytest.mark.parametrize("form", ["fixed_k5", "eval_mean"])
@pytest.mark.parametrize("name", list(NARROW_STACKS))
def test_gradients_of_narrow_and_unpadded_stacks_match_float64_autograd(name, form):
    """The GEMM engine as HE2RNA uses it at its narrowest: layers=[1] (an N = 1 product written into rows of 8, a K = 8 product,
    a weight gradient with n_out = 1) and layers=[5, 12] on input_dim 30 (every width zero-padded), through forward_fixed_k(x, 5)
    and through the eval-mode mean over ks = [1, 5, 20] (sq_he2rna_topk_mean_bwd with more than one k).  Loss (pred * r).sum();
    prediction, parameter gradients and the gradient w.r.t. x against autograd over oracle.he2rna_oracle in float64, at the bounds of
    test_gradients_match_reference_golden."""
    _lib.require_gpu()
    c = NARROW_STACKS[name]
    sd, x, r, refs, alive = _narrow_stack(name)
    ref = refs[form]
    # the reference itself exercises what the test is about: no gradient tensor vanishes, and every hidden unit of the first
    # layer (THE unit, for layers=[1]) is alive on some tiles and dead on others
    assert all(np.abs(v).max() > 0 for v in ref["grads"].values()) and np.abs(ref["gx"]).max() > 0 and np.isfinite(ref["pred"]).all()
    assert bool(alive.any(dim=2).any(dim=0).all()) and bool((~alive).any())
    assert bool((x[:, :, 0].max(dim=1)[0] > 0).all()) and bool((x.max(dim=1)[0] <= 0).any())
    m = HE2RNA(input_dim=c["D"], output_dim=12, layers=c["layers"], ks=NARROW_KS, dropout=0.5, device="cuda:0")
    m.load_state_dict(sd)
    m.eval()
    xg = x.cuda().requires_grad_(True)
    pred = m.forward_fixed_k(xg, 5) if form == "fixed_k5" else m(xg)
    (pred * r.cuda()).sum().backward()
    err = float(np.abs(pred.detach().cpu().numpy() - ref["pred"]).max() / np.abs(ref["pred"]).max())
    print(f"HE2RNA {name} {form}: prediction rel err {err:.2e}; " + ", ".join(
        f"{k} {np.abs(gk.cpu().numpy() - ref['grads'][k]).max() / np.abs(ref['grads'][k]).max():.2e}" for k, gk in m.grad_views(m.flat.grad).items()))
    assert err < 1e-4, err
    for k, gk in m.grad_views(m.flat.grad).items():
        g = ref["grads"][k]
        assert gk.shape == g.shape
        np.testing.assert_allclose(gk.cpu().numpy(), g, rtol=1e-4, atol=1e-4 * np.abs(g).max(), err_msg=k)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), ref["gx"], rtol=1e-4, atol=1e-4 * np.abs(ref["gx"]).max())


def test_full_size_against_oracle_and_training_step():
    """pretrain_gtex.py:102-105: layers [256, 256], ks [1, 2, 5, 10, 20, 50, 100], 2048-dim cluster features, 20 820 genes."""
    _lib.require_gpu()
    torch.manual_seed(3)
    B, D, N, G = 6, 2048, 100, 20820
    m = HE2RNA(input_dim=D, output_dim=G, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], device="cuda:0")
    x = torch.randn(B, N, D).clamp_min(-0.2)
    x[0, 80:] = 0
    xc = x.transpose(1, 2).contiguous()                        # channels x tiles, as the loops hand it over
    m.eval()
    with torch.no_grad():
        got = m(xc.cuda()).cpu()
        ref = ho.forward_eval({k: v.cpu() for k, v in m.state_dict().items()}, xc, m.ks, D)
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < 1e-4, err
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=3e-3, weight_decay=0.0)
    y = torch.randn(B, G).cuda()
    before = m.state_dict()["conv2.weight"]
    p1 = m(xc.cuda())
    loss = torch.nn.functional.mse_loss(p1, y)
    opt.zero_grad(); loss.backward(); opt.step()
    assert torch.isfinite(loss) and not torch.equal(before, m.state_dict()["conv2.weight"])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    with torch.no_grad():                                       # dropout is live in training mode
        a, b = m.forward_fixed_k(xc.cuda(), 10), m.forward_fixed_k(xc.cuda(), 10)
    assert not torch.equal(a, b)


def test_fit_loop_and_k_range(tmp_path):
    _lib.require_gpu()
    torch.manual_seed(0)
    np.random.seed(0)
    G, D, N = 12, 32, 20
    data = [(torch.rand(N, D), torch.rand(G), f"w{i}", "P") for i in range(12)]

    def coll(b):
        return torch.stack([t[0] for t in b]), torch.stack([t[1] for t in b]), np.array([t[2] for t in b]), np.array([t[3] for t in b])
    loader = torch.utils.data.DataLoader(data, batch_size=4, collate_fn=coll)
    m = HE2RNA(input_dim=D, output_dim=G, layers=[1], ks=[1, 5, 20], dropout=0.0, device="cuda:0")     # the reference's default hidden width of ONE
    preds, labels, wsis, projs = fit(m, 3e-3, loader, loader, loader, params={"max_epochs": 2, "patience": 5}, path=str(tmp_path), verbose=False)
    assert preds.shape == (12, G) and labels.shape == (12, G) and list(wsis[:2]) == ["w0", "w1"] and (preds >= 0).all()
    assert os.path.exists(os.path.join(str(tmp_path), "model.pt"))
    with pytest.raises(_lib.SequoiaHipError):                  # k > tiles: torch.topk raises in the reference
        HE2RNA(input_dim=D, output_dim=G, ks=[21], device="cuda:0").eval()(torch.rand(2, D, N).cuda())
