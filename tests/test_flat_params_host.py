"""Host-side contract of the flat-parameter models (ViS, ViT, UniViT): one fp32 buffer ``flat`` in which every reference tensor
is a slice (``_tmap``), shown to ``state_dict`` / ``load_state_dict`` under the reference's keys; head replacement of the two
aggregators on the CPU.  Constructors and ``sq_*_layout_init`` are host code: no GPU, no compute calls."""
import pytest
import torch
from torch import nn

from sequoia_pub_amd.uni import UniViT
from sequoia_pub_amd.vis import ViS
from sequoia_pub_amd.vit import ViT

MODELS = {
    "vis": lambda **kw: ViS(8, 64, 1, 1, 64, 64, 64, device="cpu", **kw),
    "vit": lambda **kw: ViT(num_outputs=8, dim=64, depth=1, heads=1, mlp_dim=128, device="cpu", **kw),
    "uni": lambda **kw: UniViT(embed_dim=128, depth=1, num_heads=2, img_size=32, **kw),
}
KINDS = sorted(MODELS)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _random_reference_dict(m, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(shape, generator=g) for k, (_, shape) in m._tmap.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_has_the_reference_keys_in_order_and_no_flat(kind):
    m = MODELS[kind]()
    sd = m.state_dict()
    assert list(sd) == list(m._tmap) and "flat" not in sd
    for k, (off, shape) in m._tmap.items():
        assert tuple(sd[k].shape) == tuple(shape)
        assert torch.equal(sd[k].reshape(-1), m.flat.detach()[off:off + _numel(shape)])
    pre = nn.ModuleDict({"agg": m}).state_dict()                    # as a submodule: the prefix goes in front of every key
    assert list(pre) == ["agg." + k for k in m._tmap]


@pytest.mark.parametrize("kind", KINDS)
def test_reference_keyed_dict_round_trips_bit_for_bit(kind):
    m = MODELS[kind]()
    sd = _random_reference_dict(m, 1)
    given = {k: v.clone() for k, v in sd.items()}
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    out = m.state_dict()
    assert list(out) == list(given)
    for k, v in given.items():
        assert out[k].dtype == torch.float32 and torch.equal(out[k], v), k


@pytest.mark.parametrize("kind", KINDS)
def test_dict_holding_flat_loads(kind):
    m = MODELS[kind]()
    flat = torch.randn(m.flat.numel(), generator=torch.Generator().manual_seed(2))
    res = m.load_state_dict({"flat": flat.clone()})
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.flat.detach(), flat)


@pytest.mark.parametrize("kind", KINDS)
def test_strict_load_reports_a_missing_key_under_its_reference_name(kind):
    m = MODELS[kind]()
    sd = _random_reference_dict(m, 3)
    gone = list(m._tmap)[-1]
    del sd[gone]
    with pytest.raises(RuntimeError, match="Missing key") as e:
        m.load_state_dict(dict(sd), strict=True)
    assert f'"{gone}"' in str(e.value) and '"flat"' not in str(e.value)
    res = m.load_state_dict(dict(sd), strict=False)                 # not strict: the rest loads, the key is named in the result
    assert res.missing_keys == [gone] and not res.unexpected_keys
    first = list(m._tmap)[0]
    assert torch.equal(m.state_dict()[first], sd[first])


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_shape_is_a_size_mismatch_and_leaves_the_buffer_alone(kind):
    m = MODELS[kind]()
    before = m.flat.detach().clone()
    sd = m.state_dict()
    bad = list(m._tmap)[1]
    sd[bad] = torch.full((_numel(m._tmap[bad][1]) + 3,), 7.0)       # longer than its slot: a write would run into the next tensor
    with pytest.raises(RuntimeError, match=f"size mismatch for {bad}"):
        m.load_state_dict(sd)
    assert torch.equal(m.flat.detach(), before)


@pytest.mark.parametrize("kind", KINDS)
def test_named_reference_tensors_are_views_of_the_buffer(kind):
    m = MODELS[kind]()
    named = list(m.named_reference_tensors())
    assert [k for k, _ in named] == list(m._tmap)
    for k, t in named:
        off, shape = m._tmap[k]
        assert tuple(t.shape) == tuple(shape)
        assert t.data_ptr() == m.flat.data_ptr() + 4 * off, k
    k, t = named[-1]
    t.fill_(3.5)                                                    # a view: the write lands in the buffer
    off, shape = m._tmap[k]
    assert bool((m.flat.detach()[off:off + _numel(shape)] == 3.5).all())


@pytest.mark.parametrize("kind", KINDS)
def test_grad_views_name_slices_of_a_flat_gradient(kind):
    m = MODELS[kind]()
    g = torch.arange(m.flat.numel(), dtype=torch.float32)
    gv = m.grad_views(g)
    assert list(gv) == list(m._tmap)
    for k, (off, shape) in m._tmap.items():
        assert tuple(gv[k].shape) == tuple(shape) and gv[k].data_ptr() == g.data_ptr() + 4 * off


@pytest.mark.parametrize("kind", ["vis", "vit"])
def test_head_replacement_on_the_cpu(kind):
    torch.manual_seed(4)
    m = MODELS[kind]()
    D = 64
    old_head = m.layout.head_ln_g
    body = m.flat.detach()[:old_head].clone()
    ln, lin = nn.LayerNorm(D), nn.Linear(D, 5)
    with torch.no_grad():
        ln.weight.normal_()
        ln.bias.normal_()
    m.linear_head = nn.Sequential(ln, lin)
    assert isinstance(m.flat, nn.Parameter) and m.flat.requires_grad and m.flat.numel() == m.layout.total
    assert torch.equal(m.flat.detach()[:old_head], body)            # everything in front of the old head, bit for bit
    assert m.cfg.num_outputs == 5
    sd = m.state_dict()
    assert list(sd) == list(m._tmap)
    assert tuple(sd["linear_head.1.weight"].shape) == (5, D)
    for key, given in (("linear_head.0.weight", ln.weight), ("linear_head.0.bias", ln.bias),
                       ("linear_head.1.weight", lin.weight), ("linear_head.1.bias", lin.bias)):
        assert torch.equal(sd[key], given.detach()), key
    assert "linear_head" not in dict(m.named_children())            # the head lives in the flat buffer, not in a submodule
