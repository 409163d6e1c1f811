"""What ViS, ViT, UniViT and HE2RNA share: their parameters are ONE flat fp32 buffer ``self.flat`` in which every tensor of the
reference class is a slice, ``self._tmap`` = reference state_dict key -> (offset, shape) in the reference's key order.  A slice is
contiguous unless ``self._pitch`` names a row pitch for its key: that tensor is ``[n_out, n_in, 1]`` with rows ``pitch >= n_in``
floats apart and padding between them (HE2RNA: ``round_up(n_in, 8)``, the rows its kernels read).  ``state_dict()`` /
``load_state_dict()`` speak the reference's keys, so its checkpoints round-trip unchanged."""
from collections import OrderedDict

import torch
import torch.nn as nn


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class FlatParams:
    """Mixin behind ``nn.Module`` (which stays first in the MRO); the class sets ``_tmap`` and calls ``_install_flat`` once."""
    _pitch = {}

    def _install_flat(self, flat, requires_grad=True):
        self.flat = nn.Parameter(flat, requires_grad=requires_grad)
        self._register_state_dict_hook(FlatParams._sd_hook)
        self._register_load_state_dict_pre_hook(self._load_hook)

    def _slices(self, flat):
        """(key, view of `flat`) per tensor: the tensor's own elements, none of the padding."""
        for k, (off, shape) in self._tmap.items():
            if k in self._pitch:
                yield k, flat[off:].as_strided(shape, (self._pitch[k], 1, 1))
            else:
                yield k, flat[off:off + numel(shape)].view(shape)

    @staticmethod
    def _sd_hook(module, state_dict, prefix, local_metadata):
        flat = state_dict.pop(prefix + "flat")
        for k, t in module._slices(flat.detach()):
            state_dict[prefix + k] = t.clone(memory_format=torch.contiguous_format)
        return state_dict

    def _load_hook(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Reference-keyed tensors are packed into a ``flat`` entry; a dict that already holds ``flat`` loads as it is."""
        if prefix + "flat" in state_dict or not any(prefix + k in state_dict for k in self._tmap):
            return
        flat = self.flat.detach().to("cpu", torch.float32).clone()
        for k, view in self._slices(flat):
            full = prefix + k
            if full not in state_dict:
                if strict:
                    missing_keys.append(full)
                continue
            t = state_dict.pop(full).detach().to("cpu", torch.float32)
            if t.shape != view.shape:
                error_msgs.append(f"size mismatch for {full}: {tuple(t.shape)} vs {tuple(view.shape)}")
                continue
            view.copy_(t)
        state_dict[prefix + "flat"] = flat

    def named_reference_tensors(self):
        """Views (not copies) of the flat buffer under the reference's parameter names."""
        return self._slices(self.flat.detach())

    def grad_views(self, gflat):
        """Views of a flat gradient (same layout as ``flat``) under the reference's parameter names."""
        return OrderedDict(self._slices(gflat))

    def padding_mask(self):
        """bool, the shape of ``flat``: True where the buffer holds no tensor's element (row padding, alignment gaps)."""
        pad = torch.ones_like(self.flat, dtype=torch.bool)
        for _, view in self._slices(pad):
            view.fill_(False)
        return pad
