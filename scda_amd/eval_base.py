"""What the streaming device evaluators (coco_eval.CocoEvaluator, map_eval.MapEvaluator) share: the device, the conversion of an add()
argument, the capacity check with the slice of the rows, and the rule that summarize() accumulates first when images were added since."""
import numpy as np
import torch

from scda_amd import native as N


class StreamingEvaluator:
    """A subclass sets self.I (max_images) and calls _init_stream(device); its add() takes its rows from _slots(B) and sets n_images; its
    accumulate() starts with _require_images() and ends with self._accumulated = self.n_images."""

    def _init_stream(self, device):
        dev = torch.device('cuda') if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise N.ScdaNativeError("%s needs a HIP device; there is no CPU path" % type(self).__name__)
        if dev.index is None:                   # 'cuda' -> the current device, so that tensors on it compare equal
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self._reset_stream()

    def _reset_stream(self):
        self.n_images, self._accumulated = 0, -1

    def _dev(self, t, name, dtype, shape):
        """a device tensor of exactly this type as it is; anything else through native.upload (allocates, does not wait for the device)"""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            t = N.upload(np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t), self.device, dtype).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s.add: %s must be %s, got %s" % (type(self).__name__, name, tuple(shape), tuple(t.shape)))
        return t

    def _slots(self, B):
        """the rows [s0, s1) of the next B images"""
        if self.n_images + B > self.I:
            raise ValueError("%s.add: %d images exceed max_images = %d" % (type(self).__name__, self.n_images + B, self.I))
        return self.n_images, self.n_images + B

    def _require_images(self):
        if self.n_images == 0:
            raise ValueError("%s.accumulate: no image was added" % type(self).__name__)

    def _ensure_accumulated(self):
        if self._accumulated != self.n_images:
            self.accumulate()
