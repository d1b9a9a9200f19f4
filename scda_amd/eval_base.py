"""What the streaming device evaluators (coco_eval.CocoEvaluator, map_eval.MapEvaluator) share: the device, the conversion of an add()
argument, the capacity check with the slice of the rows, the rule that summarize() accumulates first when images were added since, and
the merge of sharded evaluators (absorb / merge over scda_amd/csrc/eval_merge.hip, rules M1..M4 of include/scda_ops.h) for
data-parallel validation."""
import numpy as np
import torch

from scda_amd import native as N


def merge_order(world):
    """The order in which the ranks' rows are merged: the order of `cat results.txt.rank*`, i.e. of the decimal rank strings
    (0, 1, 10, 2, ..., 9 with 11 ranks)."""
    return sorted(range(int(world)), key=str)


class StreamingEvaluator:
    """A subclass sets self.I (max_images) and calls _init_stream(device); its add() takes its rows from _slots(B) and sets n_images; its
    accumulate() starts with _require_images() and ends with self._accumulated = self.n_images.

    For absorb() / merge() it names, once: MERGE_ROWS, ((attribute, fill), ...) -- the row arrays [max_images, ...] that accumulate()
    reads, 'image_ids' among them, each with the value of an empty row (native.EVAL_FILL) --, MERGE_COUNTERS, the int32 counters that
    are summed over the shards, MERGE_RAISES_ON_DUPLICATE, and _merge_signature(), the constructor arguments that must agree; it may
    override _check_mergeable() and _apply_duplicates(first, n).  Its summarize() calls _check_merge_flags() after its host copy."""

    MERGE_ROWS = ()
    MERGE_COUNTERS = ()
    MERGE_RAISES_ON_DUPLICATE = False

    def _init_stream(self, device):
        dev = torch.device('cuda') if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise N.ScdaNativeError("%s needs a HIP device; there is no CPU path" % type(self).__name__)
        if dev.index is None:                   # 'cuda' -> the current device, so that tensors on it compare equal
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self.merge_flags = torch.zeros(4, dtype=torch.int32, device=dev)     # include/scda_ops.h: capacity, duplicates not covered, count, total
        self._merge_first = self._merge_ws = None
        self._absorbed = False
        self._reset_stream()

    def _reset_stream(self):
        self.n_images, self._accumulated = 0, -1
        self._merged = False
        if self._absorbed:
            self.merge_flags.zero_()
            self._absorbed = False

    def _dev(self, t, name, dtype, shape):
        """a device tensor of exactly this type as it is; anything else through native.upload (allocates, does not wait for the device)"""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            t = N.upload(np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t), self.device, dtype).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s.add: %s must be %s, got %s" % (type(self).__name__, name, tuple(shape), tuple(t.shape)))
        return t

    def _slots(self, B):
        """the rows [s0, s1) of the next B images"""
        if self._merged:
            raise ValueError("%s.add: the evaluator holds merged rows; reset() it first" % type(self).__name__)
        if self.n_images + B > self.I:
            raise ValueError("%s.add: %d images exceed max_images = %d" % (type(self).__name__, self.n_images + B, self.I))
        return self.n_images, self.n_images + B

    def _require_images(self):
        if self.n_images == 0:
            raise ValueError("%s.accumulate: no image was added" % type(self).__name__)

    def _ensure_accumulated(self):
        if self._accumulated != self.n_images:
            self.accumulate()

    # ------------------------------------------------------------------------------------------------ sharded evaluators
    def _merge_signature(self):
        raise NotImplementedError

    def _check_mergeable(self):
        pass

    def _apply_duplicates(self, first, n):
        pass

    def _check_merge_flags(self):
        """after summarize()'s host copy (the device is idle): the flags the merge raised on the device"""
        if not self._absorbed:
            return
        f = self.merge_flags.cpu().numpy()
        name = type(self).__name__
        if f[0]:
            raise ValueError("%s: the merged images exceed max_images = %d" % (name, self.I))
        if f[1]:
            raise ValueError("%s: %s: not covered" % (name, "duplicate image id after the merge (shards must be unpadded)"
                                                   if self.MERGE_RAISES_ON_DUPLICATE else "duplicate image with different detections"))

    def _place(self, rows, counters, counts, order, start):
        """rows {attribute: [W, cap, ...]}, counters {attribute: int32 [W, n]}, counts: W host integers or an int32 [W] device tensor"""
        W = int(next(iter(rows.values())).shape[0])
        order = list(range(W)) if order is None else [int(o) for o in order]
        if sorted(order) != list(range(W)):
            raise ValueError("%s: order must be a permutation of the %d shards" % (type(self).__name__, W))
        on_device = torch.is_tensor(counts)
        if not on_device:
            counts = [int(c) for c in counts]
            if start + sum(counts) > self.I:
                raise ValueError("%s: %d merged images exceed max_images = %d" % (type(self).__name__, start + sum(counts), self.I))
        self._absorbed = True
        for name, fill in self.MERGE_ROWS:
            N.eval_place_rows(rows[name], order, counts, start, getattr(self, name), self.merge_flags, fill)
        for name in self.MERGE_COUNTERS:
            N.eval_sum_counters(counters[name], getattr(self, name).view(-1))
        # device counts: every slot is written, empty rows behind the total, and max_images stands for the count nobody waited for
        self.n_images, self._accumulated = (self.I if on_device else start + sum(counts)), -1
        n = self.n_images
        if n == 0:
            return
        if self._merge_first is None:
            self._merge_first = torch.empty(self.I, dtype=torch.int32, device=self.device)
            self._merge_ws = torch.empty(max(N.eval_mark_duplicates_workspace_bytes(self.I), 16), dtype=torch.uint8, device=self.device)
        N.eval_mark_duplicates(self.image_ids, n, self._merge_ws, self._merge_first, self.merge_flags, self.MERGE_RAISES_ON_DUPLICATE)
        self._apply_duplicates(self._merge_first, n)

    @torch.no_grad()
    def absorb(self, shards, order=None):
        """Appends the rows of other evaluators (same type, constructor arguments and device) behind the rows this one holds, shard by
        shard in `order` (a permutation of range(len(shards)); default: as given), sums their counters into this one's and marks the
        images whose id occurred earlier.  Not collective: for one process that evaluates shards one after another.  Nothing waits for
        the host; what only the device can see is raised by summarize().  The shards stay as they are."""
        shards = list(shards)
        if not shards:
            return self
        self._check_mergeable()
        for s in shards:
            if type(s) is not type(self) or s.device != self.device or s._merge_signature() != self._merge_signature():
                raise ValueError("%s.absorb: a shard of another type, device or constructor arguments" % type(self).__name__)
            if s is self:
                raise ValueError("%s.absorb: an evaluator cannot absorb itself" % type(self).__name__)
            s._check_mergeable()
        cap = max(1, max(s.n_images for s in shards))
        rows = {name: torch.stack([getattr(s, name)[:cap] for s in shards]) for name, _ in self.MERGE_ROWS}
        counters = {name: torch.stack([getattr(s, name).reshape(-1) for s in shards]) for name in self.MERGE_COUNTERS}
        self._place(rows, counters, [s.n_images for s in shards], order, self.n_images)
        return self

    @torch.no_grad()
    def merge(self, group=None, shard_capacity=None):
        """Collective over `group` (default: the world): gathers every rank's live rows and counters and leaves EVERY rank's evaluator
        holding all ranks' rows in merge_order(world), the counters summed; accumulate() and summarize() then run as ever, and add()
        raises until reset().  All ranks construct the evaluator with the same arguments; max_images is the capacity of the MERGED set.
        shard_capacity (default max_images): the image slots gathered from each rank, at least the largest shard --
        ceil(len(dataset) / world) for a DistributedSampler; a smaller value moves and holds fewer bytes.

        Transport.  A backend that gathers device tensors ('nccl', which is RCCL here): device all-gathers, the ranks' image counts
        included, so no rank waits for its device between its last add() and summarize(); the merged count then lives on the device
        only, every slot up to max_images is written (empty rows behind the total) and accumulate() runs over max_images images.
        Any other backend (gloo cannot gather device tensors): the rows are staged through pinned host memory, which costs ONE wait
        for the device, and the counts are known on the host.  Without an initialised process group this is a merge of one rank."""
        import torch.distributed as dist
        live = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size(group) if live else 1
        name = type(self).__name__
        cap = self.I if shard_capacity is None else int(shard_capacity)
        if not 1 <= cap <= self.I or self.n_images > cap:
            raise ValueError("%s.merge: shard_capacity must be in 1..max_images and hold this rank's %d images" % (name, self.n_images))
        if world > N.MAX_SHARDS:
            raise ValueError("%s.merge: at most %d ranks" % (name, N.MAX_SHARDS))
        if self._merged:
            raise ValueError("%s.merge: merged already; reset() first" % name)
        self._check_mergeable()
        local = {a: getattr(self, a)[:cap] for a, _ in self.MERGE_ROWS}
        local.update({a: getattr(self, a).reshape(-1) for a in self.MERGE_COUNTERS})
        mine = np.asarray([self.n_images], dtype=np.int32)
        if not live:
            gathered = {a: t.unsqueeze(0).clone() for a, t in local.items()}
            counts = [self.n_images]
        elif dist.get_backend(group) == 'nccl':
            counts = torch.empty(world, dtype=torch.int32, device=self.device)
            dist.all_gather_into_tensor(counts, N.upload(mine, self.device), group=group)
            gathered = {}
            for a, t in local.items():
                out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=self.device)
                dist.all_gather_into_tensor(out.view((world * t.shape[0],) + tuple(t.shape[1:])), t.contiguous(), group=group)
                gathered[a] = out
        else:
            host = {a: torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for a, t in local.items()}
            torch.cuda.current_stream(self.device).synchronize()             # the one wait of the staged path
            host['_counts'] = torch.from_numpy(mine)
            gathered = {}
            for a, t in host.items():
                outs = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(outs, t, group=group)
                gathered[a] = torch.stack(outs)
            counts = [int(c) for c in gathered.pop('_counts').reshape(-1)]
            gathered = {a: N.upload(t, self.device) for a, t in gathered.items()}
        for a in self.MERGE_COUNTERS:
            getattr(self, a).zero_()
        self._reset_stream()
        self._place({a: gathered[a] for a, _ in self.MERGE_ROWS}, {a: gathered[a] for a in self.MERGE_COUNTERS}, counts,
                    merge_order(world), 0)
        self._merged = True
        return self
