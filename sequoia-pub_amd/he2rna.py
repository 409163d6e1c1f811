"""HE2RNA -- the benchmark comparator of the reference (``src/he2rna.py:42-106``, built by
``src/pretrain_gtex.py:102-105`` as ``HE2RNA(input_dim, layers=[256, 256], ks=[1, 2, 5, 10, 20, 50, 100], output_dim)``)
on the HIP engine: same constructor, ``state_dict`` keys (``conv{i}.weight [out, in, 1]``, ``conv{i}.bias``),
``forward`` / ``forward_fixed_k`` / ``conv`` semantics and HuggingFace mixin, plus the loops ``training_epoch``,
``evaluate``, ``he2rna_predict`` and ``fit`` (he2rna.py:108-318).

Device path (fp32): the 1x1 Conv1d layers run as ``sq_linear`` on the token-major tensor [B * N, C] (the layout the
cluster features have BEFORE the reference's ``rearrange('b c f -> b f c')``), bias + ReLU fused; tile mask, masking,
top-k over the tiles and the position-weighted mean of he2rna.py:93-99 -- for all ``ks`` of the eval-mode mean in ONE
launch -- are ``sq_he2rna_tile_mask`` / ``sq_he2rna_topk_mean``; the backward pass is ``sq_he2rna_topk_mean_bwd``,
``sq_linear`` on transposed weights and ``sq_linear_weight_grad``.  Dropout masks are drawn with torch's device RNG
(no stream of the reference's CPU generator can be reproduced on another device anyway); everything else is C calls.
There is no CPU fallback: tensors must live on the MI355X.  The parameters are one flat fp32 buffer (``_flat.FlatParams``) in
the padded layout of ``sq_he2rna_param_layout``; every path here reads and writes it in place.

``fit(engine="fused")`` trains on ``He2rnaTrainStep`` instead: that buffer, a gradient and Adam moments in its layout, a step = ``sq_he2rna_train_forward`` + ``sq_he2rna_train_backward`` + ``sq_adamw_step`` (csrc/he2rna_train.hip:
counter-based dropout without stored masks, one loss-head launch that ranks every column once), the validation score
from one ``sq_batch_metrics`` call.  ``fit``'s default engine, ``forward`` and the loops above are unchanged."""
import os
import time
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from . import _lib
from ._flat import FlatParams

try:
    from huggingface_hub import PyTorchModelHubMixin
except Exception:                                     # pragma: no cover
    class PyTorchModelHubMixin:  # type: ignore
        pass


def _up(n, m):
    return (n + m - 1) // m * m


def param_layout(dims):
    """sq_he2rna_param_layout for ``dims = [input_dim, *layers, output_dim]``: (weight offsets, bias offsets, total), in floats.
    Layer i's weight is ``[dims[i + 1], round_up(dims[i], 8)]`` row-major; every tensor starts on a 16-byte boundary."""
    d, n = np.asarray(dims, dtype=np.int32), len(dims) - 1
    w, b, total = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64), np.zeros(1, dtype=np.int64)
    _lib.check(_lib.lib().sq_he2rna_param_layout(d.ctypes.data, n, w.ctypes.data, b.ctypes.data, total.ctypes.data))
    return [int(v) for v in w], [int(v) for v in b], int(total[0])


def _layer_stack(xt, m, p_drop=0.0, dst=None):
    """The stack of 1x1 convolutions (he2rna.py:101-106) of model `m` on token-major rows xt f32 [M, C], of which the last
    ``m.input_dim`` channels go in (:102): ``sq_linear`` per layer on the weight and bias slices of ``m.flat``, bias and ReLU fused on
    all layers but the last, dropout behind every hidden layer when p_drop > 0 (one torch.rand [M, ld] per hidden layer, in layer
    order).  Activations are zero-padded to a multiple of 8 columns, as the weight rows of ``flat`` are: the GEMM engine wants 16-byte
    rows, and the reference's default layers=[1] has a hidden width of ONE.  `dst`: where the last layer writes (f32 [M, ld >= G]
    rows, e.g. a slice of a score table) instead of a new tensor.  Returns (acts -- the padded input and every layer's output --,
    dropout masks or None per layer): what the backward pass needs; acts[-1][:, :G] are the scores."""
    dev, flat = xt.device, m.flat.detach()
    if not xt.is_cuda or flat.device != dev:
        raise _lib.SequoiaHipError(f"HE2RNA: parameters on {flat.device}, input on {dev}: both must be on the same GPU (no CPU fallback)")
    (M, C), ws = xt.shape, m._workspace(dev)
    a = torch.zeros(M, _up(m.input_dim, 8), dtype=torch.float32, device=dev)
    a[:, :m.input_dim] = xt[:, C - m.input_dim:]
    acts, drops = [a], []
    for i in range(m.n_layers):
        n_out, k_pad = int(m.dims[i + 1]), acts[-1].shape[1]
        last = i + 1 == m.n_layers
        out = dst if last and dst is not None else torch.zeros(M, _up(n_out, 8), dtype=torch.float32, device=dev)
        _lib.call("sq_linear", dev, _lib.SQ_F32, acts[-1], k_pad, flat[m.w_off[i]:], k_pad, flat[m.b_off[i]:], None, 0, _lib.SQ_F32,
                  0 if last else 2, out, _lib.SQ_F32, out.shape[1], M, n_out, k_pad, workspace=ws)
        dm = None
        if not last and p_drop > 0.0:
            dm = (torch.rand(M, out.shape[1], device=dev) >= p_drop).to(torch.float32) / (1.0 - p_drop)
            out.mul_(dm)
        drops.append(dm)
        acts.append(out)
    return acts, drops


class _He2rnaFn(torch.autograd.Function):
    """x [B, C, N] f32 -> [B, G]: forward_fixed_k for one k (scale 1) or the eval mean over ks (scale 1 / len(ks)).  The gradient
    w.r.t. the parameters is ONE tensor in the layout of ``flat``, zeroed on every backward (so its padding is exactly 0), into
    whose slices sq_linear_weight_grad writes dW and db."""

    @staticmethod
    def forward(ctx, flat, x, m, ks, scale, p_drop):
        dev, (B, C, N) = x.device, x.shape
        M = B * N
        xt = x.detach().to(torch.float32).transpose(1, 2).contiguous().view(M, C)        # free when x came from 'b c f -> b f c'
        ks_arr = np.asarray(ks, dtype=np.int32)
        mask = torch.empty(M, dtype=torch.float32, device=dev)
        _lib.call("sq_he2rna_tile_mask", dev, xt, M, C, mask)
        acts, drops = _layer_stack(xt, m, p_drop)
        pred = torch.empty(B, m.output_dim, dtype=torch.float32, device=dev)
        _lib.call("sq_he2rna_topk_mean", dev, acts[-1], acts[-1].shape[1], mask, ks_arr, len(ks_arr), float(scale), pred, B, N, m.output_dim)
        ctx.save_for_backward(flat)                    # autograd refuses the backward pass if the buffer was written in between
        ctx.saved = (acts, drops, mask, ks_arr, float(scale), (B, C, N), (m.dims, m.w_off, m.b_off), m._workspace(dev))
        return pred

    @staticmethod
    def backward(ctx, gout):
        dev, (flat,) = gout.device, ctx.saved_tensors
        acts, drops, mask, ks_arr, scale, (B, C, N), (dims, w_off, b_off), ws = ctx.saved
        M, input_dim, G = B * N, int(dims[0]), int(dims[-1])
        gflat = torch.zeros_like(flat)
        dy = torch.zeros_like(acts[-1])
        _lib.call("sq_he2rna_topk_mean_bwd", dev, acts[-1], acts[-1].shape[1], mask, ks_arr, len(ks_arr), scale,
                  gout.detach().float().contiguous(), dy, dy.shape[1], B, N, G)
        for i in range(len(w_off) - 1, -1, -1):
            a_in, n_out = acts[i], int(dims[i + 1])
            k_pad = a_in.shape[1]
            _lib.call("sq_linear_weight_grad", dev, _lib.SQ_F32, dy, dy.shape[1], a_in, k_pad, gflat[w_off[i]:], k_pad, gflat[b_off[i]:],
                      n_out, k_pad, M, workspace=ws)
            if i > 0 or ctx.needs_input_grad[1]:
                wt = torch.zeros(k_pad, dy.shape[1], dtype=torch.float32, device=dev)      # W^T, contraction over the padded outputs
                wt[:, :n_out] = flat[w_off[i]:w_off[i] + n_out * k_pad].view(n_out, k_pad).t()
                dx = torch.empty(M, k_pad, dtype=torch.float32, device=dev)
                _lib.call("sq_linear", dev, _lib.SQ_F32, dy, dy.shape[1], wt, wt.shape[1], None, None, 0, _lib.SQ_F32, 0,
                          dx, _lib.SQ_F32, k_pad, M, k_pad, dy.shape[1], workspace=ws)
                if i > 0:
                    dx.mul_((a_in > 0).to(torch.float32))          # ReLU (a dropped unit is 0 here and gets no gradient either way)
                    if drops[i - 1] is not None:
                        dx.mul_(drops[i - 1])
                dy = dx
        gx = None
        if ctx.needs_input_grad[1]:
            gx = torch.zeros(B, N, C, dtype=torch.float32, device=dev)
            gx[:, :, C - input_dim:] = dy[:, :input_dim].view(B, N, input_dim)
            gx = gx.transpose(1, 2)
        return gflat, gx, None, None, None, None


class _ScoresFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, x, m, p_drop):
        B, C, N = x.shape
        xt = x.detach().to(torch.float32).transpose(1, 2).contiguous().view(B * N, C)
        acts, _ = _layer_stack(xt, m, p_drop)
        return acts[-1][:, :m.output_dim].reshape(B, N, m.output_dim).transpose(1, 2)

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError("HE2RNA.conv is an inspection helper; train through forward / forward_fixed_k")


class HE2RNA(nn.Module, FlatParams, PyTorchModelHubMixin):
    """he2rna.py:42-106.  ``nonlin`` other than ReLU is not supported on the device path (the reference never passes one).

    The parameters are ONE fp32 buffer ``flat`` in the layout of ``param_layout`` (zero-padded weight rows), which the layer stack, the
    autograd function and He2rnaTrainStep read and write in place.  What differs from the reference class: ``parameters()`` yields
    the single ``flat`` -- the reference's names and shapes are those of ``state_dict()`` (copies), ``named_reference_tensors()``
    (views) and ``grad_views(flat.grad)`` --; there are no ``conv{i}`` attributes (a whole-module pickle that has them still loads);
    more than SQ_HE2RNA_MAX_LAYERS (8) layers are refused at construction, with the library's message; and constructing one needs
    the built library, also on the CPU (the layout is the library's)."""

    def __init__(self, input_dim, output_dim, layers=[1], nonlin=None, ks=[10], dropout=0.5, device="cpu", bias_init=None, **kwargs):
        super().__init__()
        if nonlin is not None and not isinstance(nonlin, nn.ReLU):
            raise NotImplementedError("HE2RNA on the HIP engine fuses ReLU into the layer launches; other activations are not implemented")
        self.input_dim, self.output_dim = input_dim, output_dim
        dims = [input_dim] + list(layers) + [output_dim]
        # the reference's containers, drawn in its order (the same RNG stream, the same initial values), then packed and dropped
        convs = [nn.Conv1d(dims[i], dims[i + 1], kernel_size=1, stride=1, bias=True) for i in range(len(dims) - 1)]
        pairs = [(c.weight, c.bias) for c in convs]
        if bias_init is not None:
            pairs[-1] = (pairs[-1][0], torch.as_tensor(bias_init))
        self._install_flat(self._pack(pairs))
        self.ks, self.p_drop, self.device, self._ws = np.array(ks), float(dropout), device, None
        self.to(device)

    def _pack(self, pairs):
        """(weight [n_out, n_in, 1], bias [n_out]) per layer -> sets the layout of those widths and returns a buffer in it that holds
        the tensors (padding zero), on the first weight's device."""
        dims = [pairs[0][0].shape[1]] + [w.shape[0] for w, _ in pairs]
        self.dims, self.n_layers = np.asarray(dims, dtype=np.int32), len(pairs)
        self.w_off, self.b_off, total = param_layout(dims)
        self._tmap, self._pitch = OrderedDict(), {}
        for i in range(self.n_layers):
            self._tmap[f"conv{i}.weight"] = (self.w_off[i], (dims[i + 1], dims[i], 1))
            self._tmap[f"conv{i}.bias"] = (self.b_off[i], (dims[i + 1],))
            self._pitch[f"conv{i}.weight"] = _up(dims[i], 8)
        flat = torch.zeros(total, dtype=torch.float32, device=pairs[0][0].device)
        for (_, view), t in zip(self._slices(flat), (t for pair in pairs for t in pair)):
            view.copy_(t.detach().reshape(view.shape))
        return flat

    def _workspace(self, dev):
        if self._ws is None or self._ws.device != dev:
            self._ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
        return self._ws

    def __getstate__(self):
        """``torch.save(model)`` (he2rna.py:261 pickles the whole module): the 64 MiB device workspace is scratch, not state."""
        return dict(self.__dict__, _ws=None)

    def __setstate__(self, state):
        """A whole-module pickle written before the parameters moved into ``flat`` holds ``conv{i}`` submodules: they are packed."""
        super().__setstate__(state)
        if "flat" not in self._parameters:
            convs = [self._modules.pop("conv" + str(i)) for i in range(self.n_layers)]
            self._install_flat(self._pack([(c.weight, c.bias) for c in convs]))

    def _run(self, x, ks, scale, training):
        _lib.require_gpu()
        if not x.is_cuda:
            raise _lib.SequoiaHipError("HE2RNA needs CUDA tensors (no CPU fallback)")
        if x.dim() != 3 or x.shape[1] < self.input_dim:
            raise ValueError(f"HE2RNA: x must be [batch, channels >= {self.input_dim}, tiles], got {tuple(x.shape)}")
        return _He2rnaFn.apply(self.flat, x, self, tuple(int(k) for k in ks), scale, self.p_drop if training else 0.0)

    def forward(self, x):
        if self.training:
            k = int(np.random.choice(self.ks))              # he2rna.py:85
            return self._run(x, [k], 1.0, True)
        return self._run(x, self.ks, 1.0 / len(self.ks), False)        # the mean over ks (:88-91) in one launch

    def forward_fixed_k(self, x, k):
        return self._run(x, [int(k)], 1.0, self.training)

    TILE_ROWS = 16384      # rows per launch of tile_scores: 16 384 x 20 824 x 4 B stays below the 2 GiB buffer-descriptor limit

    @torch.no_grad()
    def tile_scores(self, cache):
        """The per-tile half of forward_fixed_k (he2rna.py:93-96, :101-106) for a tile-feature cache f32 [n_tiles, C] on the
        device: the MLP is a stack of 1x1 convolutions and the mask a max over a tile's channels, so neither depends on the
        window (slide) a tile sits in.  Returns (scores f32 [n_tiles, ld >= G] -- the last layer's output on the
        ``x[:, C - input_dim:]`` channel slice of :102, columns >= G unspecified --, mask f32 [n_tiles] = max_c cache[t, c] > 0).
        Rows go through in launches of TILE_ROWS on a fixed grid (the same launches on every rank: the same bits)."""
        _lib.require_gpu()
        if not cache.is_cuda or cache.dim() != 2 or cache.shape[1] < self.input_dim:
            raise ValueError(f"HE2RNA.tile_scores: expected a device cache [n_tiles, channels >= {self.input_dim}], got {tuple(cache.shape)}")
        dev, x = cache.device, cache.to(torch.float32).contiguous()
        n, C = x.shape
        mask = torch.empty(n, dtype=torch.float32, device=dev)
        scores = torch.empty(n, _up(self.output_dim, 8), dtype=torch.float32, device=dev)
        if n == 0:
            return scores, mask
        _lib.call("sq_he2rna_tile_mask", dev, x, n, C, mask)
        for r0 in range(0, n, self.TILE_ROWS):
            r1 = min(n, r0 + self.TILE_ROWS)
            _layer_stack(x[r0:r1], self, dst=scores[r0:r1])
        return scores, mask

    def window_predictions(self, scores, mask, members):
        """Eval-mode predictions (the mean over ``ks``, he2rna.py:88-91) of windows whose tile n is row members[w, n] of a
        ``tile_scores`` table (int32 [W, N], -1 = zero padding): sq_he2rna_window_topk_mean.  Returns f32 [W, G]."""
        _lib.require_gpu()
        (W, N), G = members.shape, self.output_dim
        if members.dtype != torch.int32 or not members.is_contiguous() or scores.shape[1] < G or mask.shape[0] != scores.shape[0]:
            raise ValueError("window_predictions: members must be contiguous int32 [W, N] and scores / mask a tile_scores table")
        ks = np.asarray(self.ks, dtype=np.int32)
        out = torch.empty(W, G, dtype=torch.float32, device=scores.device)
        if W == 0:
            return out
        _lib.call("sq_he2rna_window_topk_mean", scores.device, scores, scores.shape[1], mask, scores.shape[0], members, ks, len(ks),
                  1.0 / len(ks), out, W, N, G)
        return out

    def conv(self, x):
        """Per-tile scores [B, G, N] (he2rna.py:101-106); the fused forward never materialises this layout."""
        return _ScoresFn.apply(self.flat, x, self, self.p_drop if self.training else 0.0)

    def replace_head(self, n_genes):
        """The ``--change_num_genes`` step of the k-fold experiment (he2rna.py:403-409): a fresh ``Conv1d(layers[-1], n_genes, 1)``
        becomes the last layer, for fine-tuning a model that was trained on another gene list.  ``flat`` is rebuilt in the new
        layout; every layer in front of the head keeps its bits."""
        body = [t for _, t in self.named_reference_tensors()][:-2]
        head = nn.Conv1d(int(self.dims[-2]), int(n_genes), kernel_size=1, stride=1, bias=True).to(self.flat.device)
        self.flat = nn.Parameter(self._pack(list(zip(body[0::2], body[1::2])) + [(head.weight, head.bias)]))
        self.output_dim = int(n_genes)
        return self


# ---------------------------------------------------------------------------------------------
# the training step as C calls on the model's flat parameter buffer (csrc/he2rna_train.hip)
# ---------------------------------------------------------------------------------------------
class He2rnaTrainStep:
    """One training step of he2rna.py:108-127 -- forward, MSE loss, backward, Adam -- as three C calls
    (sq_he2rna_train_forward, sq_he2rna_train_backward, sq_adamw_step) on flat fp32 buffers: the model's own ``flat`` is trained
    in place (so ``state_dict()``, ``torch.save(model)`` and ``evaluate`` see the current values at any time); the step owns the
    gradient and the two Adam moments in the same layout, its workspace and its counters.  The arithmetic of the update is
    ``torch.optim.Adam(lr, betas, eps, weight_decay=0.)``.  The model has to be on its device before the step is built; once the
    model owns another buffer (``model.to(...)`` elsewhere, ``replace_head``) the step refuses to run.

    Dropout needs no stored mask: unit (row, column) of hidden layer i is kept in step s when Philox4x32-10, keyed by
    ``seed``, says so for (s, i, row, column); ``step_index`` is the s of the next step."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, seed=0):
        _lib.require_gpu()
        if not model.flat.is_cuda:
            raise _lib.SequoiaHipError("He2rnaTrainStep needs the model on the GPU (no CPU fallback)")
        self.model, self.device = model, model.flat.device
        self.lr, self.betas, self.eps, self.seed = float(lr), (float(betas[0]), float(betas[1])), float(eps), int(seed)
        self._built_on = model.flat.detach()           # shares (and keeps alive) the memory this step's state describes
        self.total = model.flat.numel()
        self.grad, self.exp_avg, self.exp_avg_sq = (torch.zeros_like(self._built_on) for _ in range(3))
        self.t = 0                     # Adam's step count
        self.step_index = 0            # dropout stream position
        self.pred = None               # raw predictions of the last step, f32 [B, G]
        self._ws, self._shape, self._act_off = None, None, None

    @property
    def flat(self):
        """The model's parameter buffer, if it still is the one this step was built on."""
        flat = self.model.flat.detach()
        if flat.data_ptr() != self._built_on.data_ptr() or flat.numel() != self.total:
            raise _lib.SequoiaHipError("He2rnaTrainStep: the model was moved or its head replaced after this step was built; build a new step")
        return flat

    def param_views(self):
        return self.model.grad_views(self.flat)

    def grad_views(self):
        return self.model.grad_views(self.grad)

    def padding_mask(self):
        return self.model.padding_mask()

    def _workspace(self, B, N):
        if self._shape != (B, N):
            m = self.model
            off = np.zeros(m.n_layers + 1, dtype=np.int64)
            need = _lib.need(_lib.lib().sq_he2rna_train_workspace_bytes, m.dims.ctypes.data, m.n_layers, B, N, off.ctypes.data)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._shape, self._act_off = (B, N), [int(o) for o in off]
        return self._ws

    def saved_activations(self):
        """Copies of what the last step's forward pass saved: the hidden layers' outputs after ReLU and dropout, f32 [B * N, width]."""
        (B, N), dims, ws, out = self._shape, self.model.dims, self._ws.view(torch.float32), []
        for i in range(1, len(dims) - 1):
            ld = _up(int(dims[i]), 8)
            out.append(ws[self._act_off[i]:self._act_off[i] + B * N * ld].view(B * N, ld)[:, :int(dims[i])].clone())
        return out

    def forward_backward(self, x, y, k):
        """Loss (device scalar) and flat gradient of one batch at top-k `k`, without the update.  x [B, N, C] as the loader
        gives it (tiles x channels), y [B, G]."""
        dev, m, flat = self.device, self.model, self.flat
        x = x.to(dev, torch.float32).contiguous()
        y = torch.as_tensor(y).to(dev, torch.float32).contiguous()
        G = m.output_dim
        if x.dim() != 3 or x.shape[2] < m.input_dim or tuple(y.shape) != (x.shape[0], G):
            raise ValueError(f"He2rnaTrainStep: x must be [batch, tiles, channels >= {m.input_dim}] and y [batch, {G}], "
                             f"got {tuple(x.shape)} and {tuple(y.shape)}")
        B, N, C = x.shape
        ws = self._workspace(B, N)
        ks = np.asarray([int(k)], dtype=np.int32)
        self.pred = torch.empty(B, G, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("sq_he2rna_train_forward", dev, x, B, N, C, m.dims, m.n_layers, flat, ks, 1, 1.0, m.p_drop, self.seed, self.step_index,
                  y, 2.0 / (B * G), self.pred, loss, workspace=ws)
        _lib.call("sq_he2rna_train_backward", dev, B, N, m.dims, m.n_layers, flat, m.p_drop, self.grad, workspace=ws)
        return loss

    def step(self, x, y):
        """One optimisation step; returns the batch's loss as a device tensor (no host read).  The k of the step is drawn with one
        ``np.random.choice(model.ks)``, as ``HE2RNA.forward`` draws it in training mode."""
        k = int(np.random.choice(self.model.ks))              # he2rna.py:85
        loss = self.forward_backward(x, y, k)
        self.t += 1
        self.step_index += 1
        _lib.call("sq_adamw_step", self.device, self.flat, self.grad, self.exp_avg, self.exp_avg_sq, None, self.total, self.lr, self.betas[0],
                  self.betas[1], self.eps, 0.0, self.t, 1.0)
        return loss


# ---------------------------------------------------------------------------------------------
# loops (he2rna.py:108-318)
# ---------------------------------------------------------------------------------------------
def compute_correlations(labels, preds):
    """he2rna.py:140-149: mean Pearson r over the genes whose target varies, NaN r dropped."""
    rs = []
    for i in range(labels.shape[1]):
        y = labels[:, i]
        if len(np.unique(y)) > 1:
            rs.append(np.corrcoef(y, preds[:, i])[0, 1])
    rs = np.asarray(rs)
    return np.mean(rs[~np.isnan(rs)])


def _batches(model, loader):
    for x, y, wsi, proj in loader:
        x = x.float().to(model.device).transpose(1, 2)          # 'b c f -> b f c' (he2rna.py:118): channels x tiles
        yield x, y, wsi, proj


def _host_labels(y):
    """A batch's labels as a host array: the loader feed hands them over on the host, the resident feed (data.ResidentLoader) on
    the device."""
    return np.asarray(y.cpu() if torch.is_tensor(y) else y)


def training_epoch(model, dataloader, optimizer):
    """he2rna.py:108-127."""
    model.train()
    loss_fn = nn.MSELoss()
    losses = []
    for x, y, _, _ in _batches(model, dataloader):
        pred = model(x)
        loss = loss_fn(pred, y.float().to(model.device))
        losses.append(float(loss.detach()))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
    return float(np.mean(losses))


def evaluate(model, dataloader):
    """he2rna.py:151-173: validation loss on the raw predictions, correlations on ReLU(pred)."""
    model.eval()
    loss_fn = nn.MSELoss()
    losses, preds, labels = [], [], []
    with torch.no_grad():
        for x, y, _, _ in _batches(model, dataloader):
            pred = model(x)
            labels.append(_host_labels(y))
            losses.append(float(loss_fn(pred, torch.as_tensor(y).float().to(model.device))))
            preds.append(torch.relu(pred).cpu().numpy())
    preds, labels = np.concatenate(preds), np.concatenate(labels)
    return float(np.mean(losses)), compute_correlations(labels, preds)


def he2rna_predict(model, dataloader):
    """he2rna.py:175-197."""
    model.eval()
    preds, wsis, projs, labels = [], [], [], []
    with torch.no_grad():
        for x, y, wsi, proj in _batches(model, dataloader):
            preds.append(torch.relu(model(x)).cpu().numpy())
            wsis.append(wsi)
            projs.append(proj)
            labels.append(_host_labels(y))
    return np.concatenate(preds, 0), np.concatenate(labels, 0), np.concatenate(wsis, 0), np.concatenate(projs, 0)


def training_epoch_fused(trainer, dataloader):
    """training_epoch on He2rnaTrainStep: the per-batch losses stay on the device, their mean (he2rna.py:125) is read once."""
    trainer.model.train()
    losses = [trainer.step(x, y) for x, y, _, _ in dataloader]
    return float(torch.stack(losses).mean())


def device_validation_score(pred, labels):
    """``compute_correlations(labels, ReLU(pred))`` for raw predictions and labels f32 [n, G] on the device, as a device
    scalar: one sq_batch_metrics call over the whole set (fp64 Pearson r per gene, genes with a constant label skipped, NaN r
    dropped, NaN when no gene is left)."""
    lib, dev = _lib.lib(), pred.device
    n, G = pred.shape
    p = torch.relu(pred.detach().to(torch.float32)).contiguous()
    y = labels.to(dev, torch.float32).contiguous()
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.sq_train_scratch_bytes(G), dtype=torch.uint8, device=dev)
    _lib.call("sq_batch_metrics", dev, p, y, n, G, out3, scratch)
    return out3[1]


def evaluate_device(model, dataloader):
    """``evaluate`` with predictions and labels kept on the device: the loss on the raw predictions per batch, the score from
    device_validation_score over the whole validation set; two host reads per pass."""
    model.eval()
    loss_fn = nn.MSELoss()
    losses, preds, labels = [], [], []
    with torch.no_grad():
        for x, y, _, _ in _batches(model, dataloader):
            y = torch.as_tensor(y).float().to(model.device)
            pred = model(x)
            losses.append(loss_fn(pred, y))
            preds.append(pred)
            labels.append(y)
    score = device_validation_score(torch.cat(preds), torch.cat(labels))
    return float(torch.stack(losses).mean()), float(score)


def fit(model, lr, train_loader, valid_loader, test_loader, params={}, fold=None, optimizer=None, path=None, verbose=True,
        engine="autograd", seed=0):
    """he2rna.py:217-318: Adam(lr) unless an optimizer is given, up to ``max_epochs`` (200) epochs; with a validation
    loader the model with the best mean correlation is kept (``model[_fold].pt``) and training stops after ``patience``
    (100) epochs without improvement; returns the test predictions when a test loader is given, else the model.
    (The reference's wandb calls inside the validation branch reference an undefined ``args``; they are not mirrored.)
    ``engine="fused"``: the steps run on He2rnaTrainStep (Adam(lr) only: an ``optimizer`` is refused; ``seed`` keys its
    dropout) and the validation pass on evaluate_device; saving, patience and reloading follow the same rules."""
    if engine not in ("autograd", "fused"):
        raise ValueError(f"fit: engine must be 'autograd' or 'fused', got {engine!r}")
    if engine == "fused" and optimizer is not None:
        raise ValueError("fit: engine='fused' runs its own Adam(lr); it cannot take an optimizer")
    if path is not None and not os.path.exists(path):
        os.mkdir(path)
    cfg = {"max_epochs": 200, "patience": 100}
    cfg.update(params)
    if engine == "fused":
        trainer = He2rnaTrainStep(model, lr, seed=seed)
        run_epoch, run_eval = (lambda loader: training_epoch_fused(trainer, loader)), evaluate_device
    else:
        if optimizer is None:
            optimizer = torch.optim.Adam(list(model.parameters()), lr=lr, weight_decay=0.0)
        run_epoch, run_eval = (lambda loader: training_epoch(model, loader, optimizer)), evaluate
    name = "model" if fold is None else "model_" + str(fold)
    best = 0
    if valid_loader is not None:
        _, best = run_eval(model, valid_loader)
        if np.isnan(best):
            best = 0
    since_best, t0 = 0, time.time()
    try:
        for e in range(cfg["max_epochs"]):
            since_best += 1
            train_loss = run_epoch(train_loader)
            if verbose:
                print("Epoch {}/{} - {:.2f}s".format(e + 1, cfg["max_epochs"], time.time() - t0))
            t0 = time.time()
            if valid_loader is not None:
                valid_loss, score = run_eval(model, valid_loader)
                if verbose:
                    print("loss: {:.4f}, val loss: {:.4f}".format(train_loss, valid_loss))
                    print("correlations: {:.3f}".format(score))
                if score > best:
                    since_best, best = 0, score
                    if path is not None:
                        torch.save(model, os.path.join(path, name + ".pt"))
                if since_best == cfg["patience"]:
                    if verbose:
                        print("Early stopping at epoch {}".format(e + 1))
                    break
    except KeyboardInterrupt:
        pass
    if path is not None and os.path.exists(os.path.join(path, name + ".pt")):
        model = torch.load(os.path.join(path, name + ".pt"), weights_only=False)
    elif path is not None:
        torch.save(model, os.path.join(path, name + ".pt"))
    if test_loader is not None:
        return he2rna_predict(model, test_loader)
    return model
