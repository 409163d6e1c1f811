"""What ViS, ViT and UniViT share: their parameters are ONE flat fp32 buffer ``self.flat`` in which every tensor of the reference
class is a contiguous slice, ``self._tmap`` = reference state_dict key -> (offset, shape) in the reference's key order.
``state_dict()`` / ``load_state_dict()`` speak the reference's keys, so its checkpoints round-trip unchanged."""
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

    def _install_flat(self, flat, requires_grad=True):
        self.flat = nn.Parameter(flat, requires_grad=requires_grad)
        self._register_state_dict_hook(FlatParams._sd_hook)
        self._register_load_state_dict_pre_hook(self._load_hook)

    def _slices(self, flat):
        for k, (off, shape) in self._tmap.items():
            yield k, flat[off:off + numel(shape)].view(shape)

    @staticmethod
    def _sd_hook(module, state_dict, prefix, local_metadata):
        flat = state_dict.pop(prefix + "flat")
        for k, t in module._slices(flat.detach()):
            state_dict[prefix + k] = t.clone()
        return state_dict

    def _load_hook(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Reference-keyed tensors are packed into a ``flat`` entry; a dict that already holds ``flat`` loads as it is."""
        if prefix + "flat" in state_dict or not any(prefix + k in state_dict for k in self._tmap):
            return
        flat = self.flat.detach().to("cpu", torch.float32).clone()
        for k, (off, shape) in self._tmap.items():
            full = prefix + k
            if full not in state_dict:
                if strict:
                    missing_keys.append(full)
                continue
            t = state_dict.pop(full).detach().to("cpu", torch.float32)
            if tuple(t.shape) != tuple(shape):
                error_msgs.append(f"size mismatch for {full}: {tuple(t.shape)} vs {tuple(shape)}")
                continue
            flat[off:off + t.numel()] = t.reshape(-1)
        state_dict[prefix + "flat"] = flat

    def named_reference_tensors(self):
        """Views (not copies) of the flat buffer under the reference's parameter names."""
        return self._slices(self.flat.detach())

    def grad_views(self, gflat):
        """Views of a flat gradient (same layout as ``flat``) under the reference's parameter names."""
        return OrderedDict(self._slices(gflat))
