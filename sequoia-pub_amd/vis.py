"""ViS -- host-side mirror of /root/reference/src/tformer_lin.py:80-106.

Same constructor signature, ``forward([B,100,D]) -> [B,G]``, ``.device`` attribute,
``state_dict`` keys and HuggingFace ``PyTorchModelHubMixin`` behaviour as the reference
class, so ``load_state_dict`` / ``from_pretrained`` / ``torch.save(model.state_dict())``
round-trip with reference checkpoints.  All arithmetic runs in libsequoia_hip
(``sq_vis_forward`` / ``sq_vis_backward``); the parameters live in ONE flat fp32 buffer
(layout: ``sq_vis_layout_init``) in which every reference tensor is a contiguous slice.
"""
import ctypes
import math
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from ._flat import FlatParams
from ._lib import HEAD_DIM, VisConfig, VisLayout

try:  # the reference class mixes this in (tformer_lin.py:4,80)
    from huggingface_hub import PyTorchModelHubMixin
except Exception:  # pragma: no cover - hub is optional
    class PyTorchModelHubMixin:  # type: ignore
        pass


def vis_layout(cfg: VisConfig) -> VisLayout:
    lay = VisLayout()
    _lib.check(_lib.lib().sq_vis_layout_init(ctypes.byref(cfg), ctypes.byref(lay)))
    return lay


def tensor_map(cfg: VisConfig, lay: VisLayout):
    """reference state_dict key -> (offset, shape) in the flat buffer, in the reference's key order."""
    D, H, G, N = cfg.input_dim, cfg.nheads, cfg.num_outputs, cfg.num_clusters
    hd = HEAD_DIM
    m = OrderedDict()
    m["pos_emb1D"] = (lay.pos, (N, D))
    for l in range(cfg.depth):
        L = lay.layer[l]
        p = f"transformer.layers.{l}.0."
        for h in range(H):
            q = p + f"mixers.{h}."
            m[q + "local_norm.weight"] = (L.lnf_g + h * hd, (hd,))
            m[q + "local_norm.bias"] = (L.lnf_b + h * hd, (hd,))
            m[q + "summary_norm.weight"] = (L.lns_g + h * hd, (hd,))
            m[q + "summary_norm.bias"] = (L.lns_b + h * hd, (hd,))
            m[q + "s.weight"] = (L.s_w + h * hd * D, (hd, D))
            m[q + "s.bias"] = (L.s_b + h * hd, (hd,))
            m[q + "f.weight"] = (L.f_w + h * hd * D, (hd, D))
            m[q + "f.bias"] = (L.f_b + h * hd, (hd,))
            m[q + "c.weight"] = (L.c_w + h * hd * 2 * hd, (hd, 2 * hd))
            m[q + "c.bias"] = (L.c_b + h * hd, (hd,))
        m[p + "projection.weight"] = (L.proj_w, (D, H * hd))
        m[p + "projection.bias"] = (L.proj_b, (D,))
        p = f"transformer.layers.{l}.1.net."
        m[p + "0.weight"] = (L.ffln_g, (D,))
        m[p + "0.bias"] = (L.ffln_b, (D,))
        m[p + "1.weight"] = (L.ff1_w, (D, D))
        m[p + "1.bias"] = (L.ff1_b, (D,))
        m[p + "3.weight"] = (L.ff2_w, (D, D))
        m[p + "3.bias"] = (L.ff2_b, (D,))
    m["linear_head.0.weight"] = (lay.head_ln_g, (D,))
    m["linear_head.0.bias"] = (lay.head_ln_b, (D,))
    m["linear_head.1.weight"] = (lay.head_w, (G, D))
    m["linear_head.1.bias"] = (lay.head_b, (G,))
    return m


def pack_state_dict(sd, cfg: VisConfig, lay: VisLayout = None, tmap=None):
    """reference-keyed state_dict -> flat fp32 CPU tensor."""
    lay = lay or vis_layout(cfg)
    tmap = tmap or tensor_map(cfg, lay)
    flat = torch.zeros(lay.total, dtype=torch.float32)
    for k, (off, shape) in tmap.items():
        t = torch.as_tensor(sd[k]).detach().to("cpu", torch.float32)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{k}: shape {tuple(t.shape)} != expected {tuple(shape)}")
        flat[off:off + t.numel()] = t.reshape(-1)
    return flat


class _VisFunction(torch.autograd.Function):
    """forward = sq_vis_forward; backward = sq_vis_backward (grads w.r.t. the flat buffer and x)."""

    @staticmethod
    def forward(ctx, flat, x, module, need_grad):
        out = module._run_forward(x, save=need_grad)
        ctx.saved_gen = module._saved_gen if need_grad else None     # which saving forward this node belongs to
        ctx.module = module
        ctx.need_x_grad = x.requires_grad
        ctx.batch = x.shape[0]
        ctx.x_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        module = ctx.module
        if ctx.saved_gen is None or ctx.saved_gen != module._saved_gen:
            # the activations live in ONE per-module workspace: a later forward (another micro-batch, an eval pass with
            # a different batch size, ...) has overwritten what this node saved -- refuse instead of returning garbage
            raise RuntimeError("ViS.backward: the saved activations of this forward were overwritten by a later forward "
                               "of the same module; call backward() before the next grad-enabled forward "
                               "(one forward in flight per module)")
        gflat, gx = module._run_backward(grad_out.contiguous(), ctx.batch, ctx.need_x_grad)
        if gx is not None:
            gx = gx.reshape(ctx.x_shape)
        return gflat, gx, None, None


class ViS(nn.Module, FlatParams, PyTorchModelHubMixin):
    """Drop-in for the reference ``ViS`` (tformer_lin.py:80-106); see module docstring.

    Extra keyword ``compute_dtype``: ``"fp32"`` (exact-fp32 MFMA, parity mode, default) or
    ``"bf16"`` (bf16 MFMA with fp32 accumulation and fp32 residual stream, perf mode).
    """
    # What the ViT baseline (vit.py) overrides: C entry points, layout / tensor-map functions, the model width, and which of
    # the optional device paths exist
    _C_WS, _C_FWD, _C_FWD_EX = "sq_vis_workspace_bytes", "sq_vis_forward", "sq_vis_forward_ex"
    _C_BWS, _C_BWD = "sq_vis_backward_workspace_bytes", "sq_vis_backward"
    _layout_fn, _tmap_fn = staticmethod(vis_layout), staticmethod(tensor_map)
    has_tile_projection = True      # layer 0's local projection is linear in the tile feature: tile_projections / sq_vis_forward_tiles
    has_grad_buckets = True         # the backward pass reports gradient buckets as they become final: sq_vis_backward_buckets
    _saved_gen = 0                  # generation of the activations saved in the slot-0 workspace (_VisFunction.backward's guard)

    def _dim(self):
        return self.cfg.input_dim

    def __init__(self, num_outputs, input_dim, depth, nheads,
                 dimensions_f, dimensions_s, dimensions_c,
                 num_clusters=100, device='cuda:0', compute_dtype='fp32'):
        super().__init__()
        if not (dimensions_f == dimensions_s == dimensions_c == HEAD_DIM):
            raise ValueError("the HIP kernels are specialised for dimensions_f = dimensions_s = dimensions_c = 64 "
                             "(the value every reference call site uses: src/main.py:147,167,202)")
        # Same RNG draw order as the reference constructor (tformer_lin.py:86-94: pos-emb randn, then
        # per layer per head s, f, c Linear, projection, FF Linears, head Linear) so that
        # torch.manual_seed(s); ViS(...) gives the reference's initial weights.
        flat, put = self._begin(VisConfig(int(input_dim), int(depth), int(nheads), int(num_outputs), int(num_clusters)),
                                compute_dtype, device)
        put("pos_emb1D", torch.randn(num_clusters, input_dim))
        hd = HEAD_DIM
        for l in range(depth):
            p = f"transformer.layers.{l}.0."
            for h in range(nheads):
                q = p + f"mixers.{h}."
                for name, (o, i) in (("s", (hd, input_dim)), ("f", (hd, input_dim)), ("c", (hd, 2 * hd))):
                    lin = nn.Linear(i, o)
                    put(q + name + ".weight", lin.weight)
                    put(q + name + ".bias", lin.bias)
                put(q + "local_norm.weight", torch.ones(hd))
                put(q + "summary_norm.weight", torch.ones(hd))
            lin = nn.Linear(nheads * hd, input_dim)
            put(p + "projection.weight", lin.weight)
            put(p + "projection.bias", lin.bias)
            p = f"transformer.layers.{l}.1.net."
            put(p + "0.weight", torch.ones(input_dim))
            for idx in ("1", "3"):
                lin = nn.Linear(input_dim, input_dim)
                put(p + idx + ".weight", lin.weight)
                put(p + idx + ".bias", lin.bias)
        put("linear_head.0.weight", torch.ones(input_dim))
        lin = nn.Linear(input_dim, num_outputs)
        put("linear_head.1.weight", lin.weight)
        put("linear_head.1.bias", lin.bias)
        self._install_flat(flat)
        self._reset_caches()

    def _set_config(self, cfg):
        self.cfg, self.layout = cfg, self._layout_fn(cfg)
        self._tmap = self._tmap_fn(cfg, self.layout)

    def _begin(self, cfg, compute_dtype, device):
        """Head of a constructor: config -> layout and tensor map; returns the zeroed CPU buffer and ``put(key, tensor)`` into it."""
        self._set_config(cfg)
        self.compute_dtype = _lib.DTYPES[compute_dtype]
        self.device = device
        flat = torch.zeros(self.layout.total, dtype=torch.float32)

        def put(key, t):
            off, _ = self._tmap[key]
            flat[off:off + t.numel()] = t.detach().reshape(-1)
        return flat, put

    def _reset_caches(self):
        """The one home of everything derived from `flat` (its size, its device, its values): dropped by the constructors and
        by replace_head, re-created on demand by whoever uses it."""
        self._lp, self._lp_version = None, -1       # bf16 shadow of `flat` (_params_lp)
        self._ws, self._ws_key = None, None         # slot-0 workspace (uint8) and what it was sized for (_workspace)
        self._ws_extra = {}                         # slot -> (workspace, key): inference forwards in flight on several streams
        self._saved_x = None
        self._saved_gen += 1                        # whatever a forward saved in the slot-0 workspace is gone
        self._bws, self._gflat = None, None         # backward workspace and flat gradient (train.vis_backward)
        self._spatial_streams = None                # window streams of spatial.sliding_window_all_genes_sharded

    # fine-tuning replaces the head (src/main.py:155-157: model.linear_head = nn.Sequential(LN, Linear))
    def __setattr__(self, name, value):
        if name == "linear_head" and isinstance(value, nn.Module):
            self.replace_head(value)
            return
        super().__setattr__(name, value)

    def replace_head(self, head):
        ln, lin = head[0], head[1]
        G, D = lin.out_features, self._dim()
        old, body = self.flat.detach(), self.layout.head_ln_g
        cfg = type(self.cfg).from_buffer_copy(self.cfg)
        cfg.num_outputs = int(G)
        self._set_config(cfg)
        lay = self.layout
        flat = torch.zeros(lay.total, dtype=torch.float32, device=old.device)
        flat[:body] = old[:body]
        flat[lay.head_ln_g:lay.head_ln_g + D] = ln.weight.detach().to(flat.device)
        flat[lay.head_ln_b:lay.head_ln_b + D] = ln.bias.detach().to(flat.device)
        flat[lay.head_w:lay.head_w + G * D] = lin.weight.detach().reshape(-1).to(flat.device)
        flat[lay.head_b:lay.head_b + G] = lin.bias.detach().to(flat.device)
        self.flat = nn.Parameter(flat)
        self._reset_caches()

    # ---- device plumbing --------------------------------------------------------------------
    def _params_lp(self):
        if self.compute_dtype != _lib.SQ_BF16:
            return None
        if self._lp is None or self._lp.device != self.flat.device or self._lp.numel() != self.flat.numel():
            self._lp = torch.empty(self.flat.numel(), dtype=torch.bfloat16, device=self.flat.device)
            self._lp_version = -1
        if self._lp_version != self.flat._version:
            _lib.call("sq_cast_f32_to_bf16", self.flat.device, self.flat, self._lp, self.flat.numel())
            self._lp_version = self.flat._version
        return self._lp

    def _workspace(self, batch, save, slot=0):
        key = (batch, bool(save), self.compute_dtype, self.flat.device)
        need = _lib.need(getattr(_lib.lib(), self._C_WS), ctypes.byref(self.cfg), self.compute_dtype, batch, int(save))
        if slot:                     # extra inference workspaces: forwards in flight on several streams
            ws, k = self._ws_extra.get(slot, (None, None))
            if ws is None or k != key or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=self.flat.device)
                self._ws_extra[slot] = (ws, key)
            return ws
        if self._ws is None or self._ws_key != key or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.flat.device)
            self._ws_key = key
        return self._ws

    def _run_forward(self, x, save, slot=0):
        _lib.require_gpu()
        if not self.flat.is_cuda:
            raise _lib.SequoiaHipError("ViS parameters are on the CPU: call .to('cuda') first (no CPU fallback)")
        x = x.detach().to(self.flat.device, torch.float32)
        x = x.reshape(x.shape[0], -1, x.shape[-1]).contiguous()      # rearrange 'b ... d -> b (...) d'
        B, N, D = x.shape
        if N != self.cfg.num_clusters or D != self._dim():
            raise ValueError(f"expected [B, {self.cfg.num_clusters}, {self._dim()}] tokens, got {tuple(x.shape)}")
        out = torch.empty(B, self.cfg.num_outputs, dtype=torch.float32, device=x.device)
        ws = self._workspace(B, save, slot)
        lp = self._params_lp()
        _lib.call(self._C_FWD, x.device, ctypes.byref(self.cfg), self.compute_dtype, self.flat, lp, x, out, B, int(save), workspace=ws)
        self._saved_x = x if save else None
        if slot == 0:           # slot-0 workspace rewritten (or re-allocated): earlier saved activations are gone
            self._saved_gen += 1
        return out

    def tile_projections(self, cache):
        """Layer 0's local projection f (tformer_lin.py:20, all heads) per TILE of a feature cache f32 [rows, D]: returns
        (f_tile f32 [rows, heads*64] = cache . Wf^T, f_pos f32 [num_clusters, heads*64] = pos_emb1D . Wf^T + bf).  f is linear in
        tile feature + position, so a window token's f(x) is f_tile[tile] + f_pos[slot] -- what sq_vis_forward_tiles gathers
        instead of running the projection over every window token (bf16 mode; the exact fp32 mode keeps the per-token product)."""
        _lib.require_gpu()
        if not self.has_tile_projection or self.compute_dtype != _lib.SQ_BF16:
            raise NotImplementedError("tile projections are the bf16 ViS sliding-window path's")
        lay, dev = self.layout, cache.device
        D, HD, N = self._dim(), self.cfg.nheads * 64, self.cfg.num_clusters
        lp = self._params_lp()
        L0, flat = lay.layer[0], self.flat.detach()
        w = lp[L0.f_w:]
        a = cache.to(torch.bfloat16).contiguous()
        pos = flat[lay.pos:lay.pos + N * D].view(N, D).to(torch.bfloat16).contiguous()
        f_tile = torch.empty(a.shape[0], HD, dtype=torch.float32, device=dev)
        f_pos = torch.empty(N, HD, dtype=torch.float32, device=dev)
        for r0 in range(0, a.shape[0], 32768):         # operand extents stay below the 2 GiB buffer-descriptor limit
            r1 = min(a.shape[0], r0 + 32768)
            _lib.call("sq_linear", dev, self.compute_dtype, a[r0:r1], D, w, D, None, None, 0, 0, 0,
                      f_tile[r0:r1], _lib.SQ_F32, HD, r1 - r0, HD, D, None, 0)
        _lib.call("sq_linear", dev, self.compute_dtype, pos, D, w, D, flat[L0.f_b:], None, 0, 0, 0, f_pos, _lib.SQ_F32, HD, N, HD, D, None, 0)
        return f_tile, f_pos

    def _run_head_inputs(self, cache, members, slot=0, tile_proj=None):
        """Sliding-window form (sq_vis_forward_ex / sq_vit_forward_ex): cache f32 [n_rows, D] on the device, members int32
        [B, num_clusters] rows of the cache per window (-1 = zero padding).  Returns the linear head's input LayerNorm(mean_tokens X)
        f32 [B, D] -- the window batch [B, num_clusters, D] is gathered inside the first kernel and the head is left to the caller
        (``apply_head``).  ``tile_proj`` = tile_projections(cache): the first layer's local projection is gathered per tile
        (sq_vis_forward_tiles; ViS only -- a ViT layer starts with LayerNorm(x + pos), which is not linear in the tile feature)."""
        _lib.require_gpu()
        if tile_proj is not None and not self.has_tile_projection:
            raise NotImplementedError("tile projections are the bf16 ViS sliding-window path's")
        N, D = self.cfg.num_clusters, self._dim()
        if members.dim() != 2 or members.shape[1] != N or cache.dim() != 2 or cache.shape[1] != D:
            raise ValueError(f"expected members [B, {N}] and a [rows, {D}] cache")
        if members.dtype != torch.int32 or not members.is_contiguous() or cache.dtype != torch.float32 or not cache.is_contiguous():
            raise ValueError("members must be contiguous int32 and the cache contiguous float32")   # both reach the kernel as raw pointers
        B = members.shape[0]
        out = torch.empty(B, D, dtype=torch.float32, device=cache.device)
        ws = self._workspace(B, False, slot)
        lp = self._params_lp()
        if tile_proj is not None:
            f_tile, f_pos = tile_proj
            if f_tile.shape != (cache.shape[0], self.cfg.nheads * 64) or f_pos.shape != (N, self.cfg.nheads * 64):
                raise ValueError("tile_proj does not belong to this cache / model")
            _lib.call("sq_vis_forward_tiles", cache.device, ctypes.byref(self.cfg), self.compute_dtype, self.flat, lp, cache, members,
                      cache.shape[0], f_tile, f_pos, out, B, workspace=ws)
        else:
            _lib.call(self._C_FWD_EX, cache.device, ctypes.byref(self.cfg), self.compute_dtype, self.flat, lp, None, cache, members,
                      cache.shape[0], None, out, B, 0, workspace=ws)
        return out

    def apply_head(self, head_in, chunk=32768):
        """linear_head[1] of the reference (tformer_lin.py:91-94,106) on already normalised inputs f32 [R, D] -> f32 [R, G],
        `chunk` rows per product (callers that shard rows over ranks pass the grid they share with the one-rank run)."""
        if not 0 < chunk <= 32768:
            raise ValueError("apply_head: chunk must be in 1..32768 (operand extents stay below the 2 GiB buffer-descriptor limit)")
        R, D = head_in.shape
        G = self.cfg.num_outputs
        lay, dev, flat = self.layout, head_in.device, self.flat.detach()
        lp = self._params_lp()
        out = torch.empty(R, G, dtype=torch.float32, device=dev)
        if lp is not None:
            a, w = head_in.to(torch.bfloat16).contiguous(), lp[lay.head_w:]
        else:
            a, w = head_in.contiguous(), flat[lay.head_w:]
        for r0 in range(0, R, chunk):
            r1 = min(R, r0 + chunk)
            _lib.call("sq_linear", dev, self.compute_dtype, a[r0:r1], D, w, D, flat[lay.head_b:], None, 0, 0, 0,
                      out[r0:r1], _lib.SQ_F32, G, r1 - r0, G, D, None, 0)
        return out

    def _run_backward(self, grad_out, batch, need_x_grad):
        from . import train as _train           # sq_vis_backward binding lives with the training step
        return _train.vis_backward(self, grad_out, batch, need_x_grad)

    def forward(self, x):
        if x.dim() == 2:
            # spatial_vis/visualize.py:82 feeds [100, D]; the reference's rearrange turns that into
            # [100, 1, D] (+ pos-emb broadcast).  We implement the intended one-window = one sample.
            x = x.unsqueeze(0)
        need_grad = torch.is_grad_enabled() and (self.flat.requires_grad or x.requires_grad)
        return _VisFunction.apply(self.flat, x, self, need_grad)

    def forward_literal_2d(self, x2d):
        """Bit-for-bit behaviour of the reference on a 2-D [100, D] input:
        output row i depends only on tile i, replicated over the 100 positions."""
        n = x2d.shape[0]
        return self.forward(x2d[:, None, :].expand(n, self.cfg.num_clusters, x2d.shape[-1]))
