"""UNI patch embedder -- host-side mirror of what /root/reference/pre_processing/compute_features_hdf5.py:62-68 builds
with timm: ``feat_model = timm.create_model("vit_large_patch16_224", img_size=224, patch_size=16, init_values=1e-5,
num_classes=0, dynamic_img_size=True)``, ``load_state_dict(torch.load(.../pytorch_model.bin))``, ``.eval()``,
``.to(device)``, ``feat_model(image) -> [1, 1024]`` (:126-129; spatial_vis/visualize.py:220-232 likewise).

``UniViT`` keeps timm's state-dict keys (``cls_token``, ``pos_embed``, ``patch_embed.proj.*``,
``blocks.{i}.{norm1,attn.qkv,attn.proj,ls1.gamma,norm2,mlp.fc1,mlp.fc2,ls2.gamma}``, ``norm.*``) so the published
``pytorch_model.bin`` loads unchanged; the parameters live in one flat fp32 buffer (``sq_uni_layout``) and all
arithmetic runs in ``sq_uni_forward`` (csrc/uni.hip).  Forward only (the reference never trains the extractor).
timm is absent from the build image: parity is against oracle/uni_oracle.py, a restatement of timm's published
algorithm ("parity unpinned")."""
import ctypes
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _abi, _lib
from ._flat import FlatParams, numel

SQ_UNI_MAX_DEPTH = _abi.CONSTANTS["SQ_UNI_MAX_DEPTH"]
UniConfig, UniLayerOffsets, UniLayout = (_abi.STRUCTS[n] for n in ("sq_uni_config", "sq_uni_layer_offsets", "sq_uni_layout"))


def tensor_map(cfg, lay):
    """timm state_dict key -> (offset, shape) in the flat buffer."""
    D, M, T = cfg.dim, cfg.mlp_dim, (cfg.img_size // 16) ** 2 + 1
    m = OrderedDict()
    m["cls_token"] = (lay.cls, (1, 1, D))
    m["pos_embed"] = (lay.pos, (1, T, D))
    m["patch_embed.proj.weight"] = (lay.patch_w, (D, 3, 16, 16))
    m["patch_embed.proj.bias"] = (lay.patch_b, (D,))
    for i in range(cfg.depth):
        L, p = lay.layer[i], f"blocks.{i}."
        m[p + "norm1.weight"] = (L.ln1_g, (D,)); m[p + "norm1.bias"] = (L.ln1_b, (D,))
        m[p + "attn.qkv.weight"] = (L.qkv_w, (3 * D, D)); m[p + "attn.qkv.bias"] = (L.qkv_b, (3 * D,))
        m[p + "attn.proj.weight"] = (L.proj_w, (D, D)); m[p + "attn.proj.bias"] = (L.proj_b, (D,))
        m[p + "ls1.gamma"] = (L.ls1, (D,))
        m[p + "norm2.weight"] = (L.ln2_g, (D,)); m[p + "norm2.bias"] = (L.ln2_b, (D,))
        m[p + "mlp.fc1.weight"] = (L.fc1_w, (M, D)); m[p + "mlp.fc1.bias"] = (L.fc1_b, (M,))
        m[p + "mlp.fc2.weight"] = (L.fc2_w, (D, M)); m[p + "mlp.fc2.bias"] = (L.fc2_b, (D,))
        m[p + "ls2.gamma"] = (L.ls2, (D,))
    m["norm.weight"] = (lay.norm_g, (D,)); m["norm.bias"] = (lay.norm_b, (D,))
    return m


def _gemm_blocks(cfg, lay):
    """(weight offset, rows, row length, bias offset) of every product of the network, in launch order."""
    D, M = cfg.dim, cfg.mlp_dim
    out = [(lay.patch_w, D, 3 * 16 * 16, lay.patch_b)]
    for i in range(cfg.depth):
        L = lay.layer[i]
        out += [(L.qkv_w, 3 * D, D, L.qkv_b), (L.proj_w, D, D, L.proj_b), (L.fc1_w, M, D, L.fc1_b), (L.fc2_w, D, M, L.fc2_b)]
    return out


def fold_layer_scale(flat, lay, cfg):
    """A copy of the flat buffer with the LayerScale gains folded into attn.proj / mlp.fc2 (weight rows and biases)."""
    w = flat.detach().clone()
    D, M = cfg.dim, cfg.mlp_dim
    for i in range(cfg.depth):
        L = lay.layer[i]
        for w_off, b_off, g_off, k in ((L.proj_w, L.proj_b, L.ls1, D), (L.fc2_w, L.fc2_b, L.ls2, M)):
            gam = w[g_off:g_off + D]
            w[w_off:w_off + D * k] = (w[w_off:w_off + D * k].view(D, k) * gam[:, None]).reshape(-1)
            w[b_off:b_off + D] = w[b_off:b_off + D] * gam
    return w


def split_exec_planes(flat, lay, cfg):
    """fp32 flat buffer -> (params_exec, bias_exec) of the split-fp16 mode (include/sequoia_hip.h, sq_uni_forward):
    LayerScale folded into proj / fc2 first; every GEMM weight row then scaled by s, the power of two that lifts its max |w'|
    into (128, 256] (1 for a zero row), so that the lo plane (<= 2^-11 of the value) stays a normal fp16 number for every weight
    that matters in the row; params_exec = fp16 hi plane [total] then lo plane [total] (as int16); bias_exec = the folded fp32
    buffer [total] then the factors 1 / s at each GEMM's bias offset [total] (1 elsewhere).  Pure tensor code: runs on CPU too."""
    w = fold_layer_scale(flat, lay, cfg)
    bias = w.clone()
    factor = torch.ones_like(w)
    for w_off, rows, k, b_off in _gemm_blocks(cfg, lay):
        blk = w[w_off:w_off + rows * k].view(rows, k)
        amax = blk.abs().amax(dim=1).double()
        s = torch.where(amax > 0, torch.exp2(torch.floor(torch.log2(256.0 / amax.clamp_min(1e-30)))), torch.ones_like(amax))
        s = s.clamp(2.0 ** -20, 2.0 ** 20).to(w.dtype)
        blk.mul_(s[:, None])                             # exact: powers of two
        factor[b_off:b_off + rows] = 1.0 / s
    # the planes of everything outside the GEMM weights are never read: zero there (no fp16 overflow of embeddings)
    mask = torch.zeros_like(w, dtype=torch.bool)
    for w_off, rows, k, _ in _gemm_blocks(cfg, lay):
        mask[w_off:w_off + rows * k] = True
    w = torch.where(mask, w, torch.zeros_like(w))
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return torch.cat([hi, lo]).view(torch.int16), torch.cat([bias, factor])


class UniViT(nn.Module, FlatParams):
    """timm VisionTransformer subset: ViT with class token, learned position embedding, LayerScale, token pooling,
    no classifier head.  ``forward(x f32 [B, 3, S, S]) -> f32 [B, dim]``."""

    def __init__(self, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0, img_size=224, patch_size=16, init_values=1e-5,
                 num_classes=0, compute_dtype="fp32", mlp_dim=None, **_ignored):
        """mlp_dim: the hidden width itself where embed_dim * mlp_ratio does not say it exactly (192 * (200 / 192) is 199.99...)."""
        super().__init__()
        if patch_size != 16 or num_classes != 0 or embed_dim != num_heads * 64:
            raise ValueError("the HIP kernels cover patch_size=16, head dim 64, num_classes=0 (the reference's UNI configuration)")
        self.cfg = UniConfig(int(embed_dim), int(depth), int(num_heads), int(embed_dim * mlp_ratio) if mlp_dim is None else int(mlp_dim),
                             int(img_size))
        self.layout = UniLayout()
        _lib.check(_lib.lib().sq_uni_layout_init(ctypes.byref(self.cfg), ctypes.byref(self.layout)))
        self._tmap = tensor_map(self.cfg, self.layout)
        self.compute_dtype = _lib.DTYPES[compute_dtype]
        if self.compute_dtype == _lib.SQ_BF16X3:
            raise ValueError("UniViT: compute_dtype 'bf16x3' is the ResNet-50 embedder's split mode; UNI's split mode is 'f16x3'")
        self._init_values = init_values
        flat = torch.zeros(self.layout.total, dtype=torch.float32)
        # timm's init: trunc_normal(std .02) embeddings / Linear weights, zero biases, LayerNorm 1 / 0, LayerScale init_values
        g = torch.Generator().manual_seed(torch.initial_seed() % (2 ** 31))
        for k, (off, shape) in self._tmap.items():
            n = numel(shape)
            if k.endswith("gamma"):
                flat[off:off + n] = init_values if init_values is not None else 1.0
            elif "norm" in k and k.endswith("weight"):
                flat[off:off + n] = 1.0
            elif k.endswith("bias"):
                pass
            else:
                flat[off:off + n] = torch.nn.init.trunc_normal_(torch.empty(n), std=0.02, generator=g)
        self._install_flat(flat, requires_grad=False)
        self._exec = None
        self._exec_key = None
        self._ws = {}

    # ---- execution copies: LayerScale folded into attn.proj / mlp.fc2 -------------------------------------------------
    def _exec_params(self):
        dev = self.flat.device
        key = (dev, self.compute_dtype, self.flat._version)
        if self._exec_key == key:
            return self._exec
        if self.compute_dtype == _lib.SQ_F16X3:
            weights_exec, bias_exec = split_exec_planes(self.flat, self.layout, self.cfg)
            self._exec, self._exec_key = (weights_exec, bias_exec), key
            return self._exec
        w = fold_layer_scale(self.flat, self.layout, self.cfg)
        bias_exec = w                                                   # fp32, folded biases (weights in it are unused)
        weights_exec = w.to(torch.bfloat16) if self.compute_dtype == _lib.SQ_BF16 else w
        self._exec, self._exec_key = (weights_exec, bias_exec), key
        return self._exec

    # ---- the reduced range of the split-fp16 mode ----------------------------------------------------------------
    def exact_twin(self):
        """The same network in the exact fp32 mode (a copy of the parameters, refreshed only when they changed): what a launch
        group is re-run in when the split-fp16 mode overflowed (an activation >= 65504; sq_uni_forward_checked)."""
        key = (self.flat.device, self.flat._version)
        tw = self.__dict__.get("_twin")
        if tw is None:
            c = self.cfg
            tw = UniViT(embed_dim=c.dim, depth=c.depth, num_heads=c.heads, mlp_dim=c.mlp_dim, img_size=c.img_size,
                        init_values=self._init_values, compute_dtype="fp32")
            self.__dict__["_twin"] = tw                  # not a registered submodule: state_dict() keeps timm's keys
            self.__dict__["_twin_key"] = None
        if self.__dict__.get("_twin_key") != key or tw.flat.device != self.flat.device:
            with torch.no_grad():
                tw.flat = nn.Parameter(self.flat.detach().clone(), requires_grad=False)
            tw._exec_key = None                          # a fresh tensor restarts its version counter: drop the twin's folded copy
            self.__dict__["_twin_key"] = key
        return tw

    def new_flag(self):
        """A zeroed device word for sq_uni_forward_checked's non-finite flag."""
        return torch.zeros(1, dtype=torch.int32, device=self.flat.device)

    def _resolve_nonfinite(self, feats, flag, on_nonfinite, rerun):
        """Read the flag (host sync); overflowed -> raise, or re-run in fp32 (`rerun()` returns the exact features)."""
        if flag is None or int(flag.item()) == 0:
            return feats
        msg = ("UniViT in split-fp16 mode (f16x3): an activation left fp16's range (>= 65504) and the features are not finite"
               " -- unusual weights")
        if on_nonfinite == "raise":
            raise _lib.SequoiaHipError(msg + "; use compute_dtype='fp32' for this checkpoint")
        import warnings
        warnings.warn(msg + "; this launch group is re-run in exact fp32", RuntimeWarning, stacklevel=3)
        self.last_nonfinite_reruns = getattr(self, "last_nonfinite_reruns", 0) + 1
        return rerun()

    def _run(self, patches_u8=None, x_f32=None, slot=0, flag=None):
        _lib.require_gpu()
        if not self.flat.is_cuda:
            raise _lib.SequoiaHipError("UniViT parameters are on the CPU: call .to('cuda') first (no CPU fallback)")
        dev = self.flat.device
        src = patches_u8 if patches_u8 is not None else x_f32
        n = src.shape[0]
        S = src.shape[1] if patches_u8 is not None else src.shape[2]
        if S != self.cfg.img_size:
            raise ValueError(f"patches are {S} x {S}, the model's position embedding is for {self.cfg.img_size} x {self.cfg.img_size}: "
                             "resize first (compute_features_hdf5.py:54 Resize(224))")
        wx, bx = self._exec_params()
        out = torch.empty(n, self.cfg.dim, dtype=torch.float32, device=dev)
        need = _lib.lib().sq_uni_workspace_bytes(ctypes.byref(self.cfg), self.compute_dtype, n)
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self._ws[slot] = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call("sq_uni_forward_checked", dev, ctypes.byref(self.cfg), self.compute_dtype, self.flat, wx, bx, patches_u8, x_f32, n, out,
                  ws, ws.numel(), flag)
        return out

    @torch.no_grad()
    def forward(self, x, on_nonfinite="rerun"):
        """timm's ``model(image)`` with num_classes=0: f32 [B, 3, S, S] (normalised) -> f32 [B, dim].  Split-fp16 mode: an
        overflow is handled per `on_nonfinite` ("rerun" / "raise", as in extract_patches_u8)."""
        x = x.to(self.flat.device, torch.float32).contiguous()
        if self.compute_dtype != _lib.SQ_F16X3:
            return self._run(x_f32=x)
        flag = self.new_flag()
        feats = self._run(x_f32=x, flag=flag)
        return self._resolve_nonfinite(feats, flag, on_nonfinite, lambda: self.exact_twin()._run(x_f32=x))

    def max_sub_batch(self, S=None):
        """Largest launch group the 2 GiB buffer-descriptor limit allows (sq_uni_forward's check): the widest activation is
        [n * tokens, max(3 dim, mlp_dim)] in the compute dtype."""
        S = S or self.cfg.img_size
        tokens = (S // 16) ** 2 + 1
        es = 4 if self.compute_dtype == _lib.SQ_F32 else 2          # f16x3: per fp16 plane
        return max(1, ((1 << 31) - 1) // (tokens * max(3 * self.cfg.dim, self.cfg.mlp_dim) * es))

    @torch.no_grad()
    def extract_patches_u8(self, patches, sub_batch=128, on_nonfinite="rerun", flag=None):
        """uint8 HWC patches [n, S, S, 3] -> f32 [n, dim]; fuses the ToTensor + Normalize of compute_features_hdf5.py:53-56.
        Launch groups of <= sub_batch patches (clamped to the descriptor limit); larger groups are faster -- the 256 x 256 GEMM
        tiles then fill more rounds (bench: 6.09 / 6.38 / 6.58 slides/s at 256 / 500 / 1000).
        Split-fp16 mode: features that came out non-finite (an activation beyond fp16's range) are, per `on_nonfinite`, re-run
        in exact fp32 with a warning ("rerun", one host sync per call), reported by an exception ("raise"), or left to the
        caller ("defer": no sync; pass `flag`, a zeroed int32 device word from new_flag(), and check it later -- SlidePipeline
        does)."""
        dev = self.flat.device
        patches = torch.as_tensor(patches)
        if patches.shape[0] == 0:
            return torch.empty(0, self.cfg.dim, dtype=torch.float32, device=dev)
        if on_nonfinite not in ("rerun", "raise", "defer"):
            raise ValueError(f"on_nonfinite={on_nonfinite!r}: 'rerun', 'raise' or 'defer'")
        sub_batch = max(1, min(int(sub_batch), self.max_sub_batch(patches.shape[1])))
        if self.compute_dtype == _lib.SQ_F16X3:
            if on_nonfinite != "defer":
                flag = self.new_flag()
                feats = self.extract_patches_u8(patches, sub_batch, "defer", flag)
                return self._resolve_nonfinite(feats, flag, on_nonfinite, lambda: self.exact_twin().extract_patches_u8(patches, sub_batch))
        else:
            flag = None
        return torch.cat([self._run(patches_u8=patches[i:i + sub_batch].to(dev).contiguous(), flag=flag)
                          for i in range(0, patches.shape[0], sub_batch)], 0)


def resize_u8(patches_u8, size=224):
    """transforms.Resize(224) of compute_features_hdf5.py:54 for a batch of uint8 HWC patches on the device: bilinear with
    anti-aliasing (what PIL's BILINEAR resampler does when shrinking), rounded back to uint8.  PIL works in fixed point
    per image; this float version can differ by one grey level."""
    x = patches_u8.permute(0, 3, 1, 2).to(torch.float32)
    y = torch.nn.functional.interpolate(x, size=(size, size), mode="bilinear", antialias=True, align_corners=False)
    return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def create_model(name="vit_large_patch16_224", img_size=224, patch_size=16, init_values=1e-5, num_classes=0, dynamic_img_size=True,
                 compute_dtype="fp32", **kw):
    """The ``timm.create_model`` call of compute_features_hdf5.py:63-64 for the one architecture the reference uses."""
    if name != "vit_large_patch16_224":
        raise ValueError(f"only vit_large_patch16_224 (UNI) is provided, not {name!r}")
    return UniViT(embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4.0, img_size=img_size, patch_size=patch_size,
                  init_values=init_values, num_classes=num_classes, compute_dtype=compute_dtype)
