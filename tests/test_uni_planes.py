"""Host-side packing of the UNI embedder's split-fp16 mode (uni.split_exec_planes): the fp16 planes and the 1 / s factors
that sq_uni_forward reads in f16x3 mode (include/sequoia_hip.h).  CPU only."""
import torch

from oracle import uni_oracle
from sequoia_pub_amd.uni import UniViT, _gemm_blocks, fold_layer_scale, split_exec_planes


def _tiny():
    cfg = dict(embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, img_size=32)
    sd = uni_oracle.init_state_dict(dim=128, depth=2, heads=2, mlp_dim=512, img_size=32, seed=3, scale_ls=0.5)
    m = UniViT(compute_dtype="f16x3", **cfg)
    m.load_state_dict(sd)
    return m, sd


def test_planes_scales_and_factors():
    m, sd = _tiny()
    lay, cfg = m.layout, m.cfg
    total = lay.total
    wx, bx = split_exec_planes(m.flat, lay, cfg)
    assert wx.dtype == torch.int16 and wx.numel() == 2 * total and bx.dtype == torch.float32 and bx.numel() == 2 * total
    hi = wx[:total].view(torch.float16).double()
    lo = wx[total:].view(torch.float16).double()
    folded = fold_layer_scale(m.flat, lay, cfg).double()
    factor_slots = torch.zeros(total, dtype=torch.bool)
    blocks = _gemm_blocks(cfg, lay)
    assert len(blocks) == 1 + 4 * cfg.depth
    for w_off, rows, k, b_off in blocks:
        inv = bx[total + b_off:total + b_off + rows].double()
        s = 1.0 / inv
        mant, _ = torch.frexp(s)
        assert torch.all(mant == 0.5), "every scale is a power of two"
        wp = folded[w_off:w_off + rows * k].view(rows, k) * s[:, None]
        rmax = wp.abs().amax(dim=1)
        assert torch.all(rmax > 128) and torch.all(rmax <= 256)
        rec = (hi[w_off:w_off + rows * k] + lo[w_off:w_off + rows * k]).view(rows, k)
        assert torch.all((rec - wp).abs() <= 2.0 ** -22 * wp.abs() + 2.0 ** -25), "hi + lo reconstructs w' to 2^-22"
        factor_slots[b_off:b_off + rows] = True
    assert torch.all(bx[total:][~factor_slots] == 1.0)
    assert torch.equal(bx[:total], fold_layer_scale(m.flat, lay, cfg))          # the first half: the folded biases


def test_layer_scale_is_folded_before_scaling():
    m, sd = _tiny()
    lay, cfg = m.layout, m.cfg
    total = lay.total
    wx, bx = split_exec_planes(m.flat, lay, cfg)
    hi = wx[:total].view(torch.float16).double()
    lo = wx[total:].view(torch.float16).double()
    for i in range(cfg.depth):
        L = lay.layer[i]
        for w_off, b_off, wkey, bkey, gkey, k in ((L.proj_w, L.proj_b, "attn.proj.weight", "attn.proj.bias", "ls1.gamma", cfg.dim),
                                                  (L.fc2_w, L.fc2_b, "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma", cfg.mlp_dim)):
            gam = sd[f"blocks.{i}.{gkey}"].double()
            w = sd[f"blocks.{i}.{wkey}"].double() * gam[:, None]
            s = 1.0 / bx[total + b_off:total + b_off + cfg.dim].double()
            rec = (hi[w_off:w_off + cfg.dim * k] + lo[w_off:w_off + cfg.dim * k]).view(cfg.dim, k) / s[:, None]
            assert float(((rec - w).abs().amax(dim=1) / w.abs().amax(dim=1)).max()) < 2.0 ** -21
            # the scale lifts the FOLDED row (gains ~0.5 here: scaling the raw row would leave the folded one in (64, 128])
            assert torch.all((w * s[:, None]).abs().amax(dim=1) > 128)
            assert torch.allclose(bx[b_off:b_off + cfg.dim].double(), sd[f"blocks.{i}.{bkey}"].double() * gam, rtol=1e-6, atol=0)


def test_split_mode_names():
    import pytest
    with pytest.raises(ValueError, match="f16x3"):
        UniViT(embed_dim=128, depth=1, num_heads=2, img_size=32, compute_dtype="bf16x3")
    m = UniViT(embed_dim=128, depth=1, num_heads=2, img_size=32, compute_dtype="f16x3")
    assert m.max_sub_batch() == UniViT(embed_dim=128, depth=1, num_heads=2, img_size=32, compute_dtype="bf16").max_sub_batch()
