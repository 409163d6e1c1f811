"""Host side of the HE2RNA training step (no GPU): the float64 reference the GPU tests compare against is itself checked
against torch, the flat parameter layout against its restatement, and the experiment script's parser against the
reference's flag list (tests/golden/he2rna_cli_flags.json)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import he2rna_train_cases as tc
from oracle import he2rna_oracle as ho
from sequoia_pub_amd import he2rna
from sequoia_pub_amd.cli import he2rna as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_float64_trajectory_reproduces_torch_adam():
    """tc.trajectory (oracle + restated Adam, k from a seeded RandomState) against torch.optim.Adam(lr, weight_decay=0.) on float64
    parameters with np.random.choice after np.random.seed: the same losses and parameters to rounding."""
    c, sd, batches = tc.case("l5x12")
    losses, final, _ = tc.reference_trajectory("l5x12")
    p = {n: v.detach().double().clone().requires_grad_(True) for n, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=tc.LR, weight_decay=0.0)
    np.random.seed(tc.K_SEED)
    for t in range(tc.STEPS):
        x, y = batches[t % 3]
        k = int(np.random.choice(np.array(c["ks"])))
        loss = F.mse_loss(ho.forward_fixed_k(p, x.double().transpose(1, 2), k, c["D"]), y.double())
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert abs(float(loss.detach()) - losses[t]) <= 1e-12 * abs(losses[t]), (t, float(loss.detach()), losses[t])
    assert losses[-1] < losses[0]
    for n in p:
        assert float((p[n].detach() - final[n]).abs().max()) <= 1e-12, n


def test_gated_forward_without_dropout_is_the_oracle_and_replay_reproduces_dropout_scaling():
    c, sd, batches = tc.case("l5x12")
    x, _ = batches[0]
    sd64 = {n: v.double() for n, v in sd.items()}
    xc = x.double().transpose(1, 2)
    ref = ho.forward_fixed_k(sd64, xc, 5, c["D"])
    h0 = F.relu(F.conv1d(xc[:, c["C"] - c["D"]:], sd64["conv0.weight"], sd64["conv0.bias"]))
    a0 = h0.transpose(1, 2).reshape(c["B"] * c["N"], -1)
    h1 = F.relu(F.conv1d(h0, sd64["conv1.weight"], sd64["conv1.bias"]))
    a1 = h1.transpose(1, 2).reshape(c["B"] * c["N"], -1)
    got = tc.forward_k(sd64, x.double(), 5, c["D"], gates=[tc.replay_gate(a0, 0.0), tc.replay_gate(a1, 0.0)])
    assert float((got - ref).abs().max()) <= 1e-14
    torch.manual_seed(3)
    h = F.relu(torch.randn(64, 40, dtype=torch.float64))
    for p in (0.25, 0.5):
        a = F.dropout(h, p, training=True)
        assert 0.1 < float(((a > 0) & (h > 0)).sum() / (h > 0).sum()) < 0.95
        assert torch.allclose(h * tc.replay_gate(a, p), a, rtol=1e-15, atol=0)


@pytest.mark.parametrize("dims", [[30, 5, 12, 12], [35, 1, 13], [32, 1, 12], [2048, 256, 256, 20820]],
                         ids=["no_multiple_of_8", "width_1_odd", "width_1", "reference"])
def test_param_layout_equals_its_restatement(dims):
    w_off, b_off, total = he2rna.param_layout(dims)
    assert (w_off, b_off, total) == tc.param_layout(dims)
    spans = []
    for i, (wo, bo) in enumerate(zip(w_off, b_off)):
        spans += [(wo, wo + dims[i + 1] * tc.up8(dims[i])), (bo, bo + dims[i + 1])]
    assert all(a % 4 == 0 for a, _ in spans) and all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])) and spans[-1][1] <= total
    if dims == [2048, 256, 256, 20820]:
        assert total == 2048 * 256 + 256 + 256 * 256 + 256 + 20820 * 256 + 20820


@pytest.mark.parametrize("dims,B,N", [([2048, 256, 256, 20820], 16, 100), ([64, 24, 40, 203], 5, 100), ([30, 5, 12, 12], 3, 20), ([32, 12], 2, 1)])
def test_step_workspace_holds_its_pieces_and_nothing_unaccounted(dims, B, N):
    """Saved activations, the gradient of the scores, two dX tables, one transposed weight, the loss partials and the 64 MiB
    split-K scratch, each rounded up to 256 bytes: the size is their sum, and the saved tables do not overlap."""
    from sequoia_pub_amd import _lib
    lib = _lib.lib()
    d = np.asarray(dims, dtype=np.int32)
    off = np.zeros(len(dims), dtype=np.int64)
    got = lib.sq_he2rna_train_workspace_bytes(d.ctypes.data, len(dims) - 1, B, N, off.ctypes.data)
    M, ld = B * N, [tc.up8(v) for v in dims]
    hid = max(ld[1:-1], default=0)
    pieces = [M] + [M * v for v in ld] + [M * ld[-1], M * hid, M * hid, max((a * b for a, b in zip(ld[1:-1], ld[2:])), default=0),
                                          lib.sq_he2rna_loss_head_workspace_bytes(B, dims[-1]) // 4, (64 << 20) // 4]
    assert got == sum((4 * p + 255) // 256 * 256 for p in pieces)
    assert all(int(o) % 64 == 0 for o in off)
    assert all(int(a) + M * w <= int(b) for a, w, b in zip(off, ld, off[1:]))
    assert lib.sq_he2rna_train_workspace_bytes(d.ctypes.data, len(dims) - 1, B, 129, None) == 0 and b"129 tiles" in lib.sq_last_error()


def test_layout_refuses_bad_dims():
    from sequoia_pub_amd import _lib
    with pytest.raises(_lib.SequoiaHipArgError, match="width 0"):
        he2rna.param_layout([32, 0, 12])
    with pytest.raises(_lib.SequoiaHipArgError, match="layers"):
        he2rna.param_layout(list(range(1, 12)))


def test_cli_parser_accepts_the_reference_flags_with_its_defaults():
    flags = json.load(open(os.path.join(GOLDEN, "he2rna_cli_flags.json")))
    parser = cli.build_parser()
    defaults = vars(parser.parse_args([]))
    for flag, spec in flags.items():
        assert defaults[flag[2:]] == spec["default"], flag
    sample = {"str": "s", "int": "7", "float": "0.25"}
    argv = []
    for flag, spec in flags.items():
        argv += [flag] if spec["type"] == "flag" else [flag, sample[spec["type"]]] + ([sample[spec["type"]]] if spec.get("nargs") else [])
    got = vars(parser.parse_args(argv))
    for flag, spec in flags.items():
        want = {"flag": True, "str": "s", "int": 7, "float": 0.25}[spec["type"]]
        assert got[flag[2:]] == ([want, want] if spec.get("nargs") else want), flag
    assert (defaults["max_epochs"], defaults["patience"], defaults["dropout"]) == (200, 100, 0.5)
    assert defaults["engine"] == "fused"      # measured not slower than autograd (profiles/he2rna_train_rate.txt)
    with pytest.raises(SystemExit):
        parser.parse_args(["--engine", "eager"])


def test_fit_refuses_an_optimizer_with_the_fused_engine_and_an_unknown_engine():
    m = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="optimizer"):
        he2rna.fit(m, 1e-3, [], None, None, optimizer=torch.optim.SGD(m.parameters(), lr=0.1), engine="fused")
    with pytest.raises(ValueError, match="engine"):
        he2rna.fit(m, 1e-3, [], None, None, engine="eager")
