"""Device-side half of the batch producer: collated CPU batches -> batches resident in HBM
without ever stalling the training stream.

The reference moves each field with its own blocking `.cuda()` inside forward (llama/model.py:255-264: ~8
pageable copies per step on the compute stream). Here a background thread packs every tensor the step reads
into ONE pinned staging buffer per slot, one asynchronous H2D copy per batch runs on a side stream, and the
consumer gets views of the slot's device buffer after a stream-side event wait (no host synchronisation).
`depth` slots are in flight; a slot is refilled only after the step that consumed it has been passed by the
compute stream. Host integers (`video_start`, `prefix_index`) stay Python lists, as the model reads them.
On a CPU device the same packing runs without pinning and streams (used by the CPU tests)."""
from __future__ import annotations

import math
import queue
import threading
from typing import Dict, Iterable, Iterator, List, Optional, Tuple

import numpy as np
import torch

_ALIGN = 256
from . import scored

# dicts over tasks (scored_*: the scored-row lists of the LM streams, fvqa/scored.py — made here, where the labels are on the host,
# so that the step's LM head can run on the scored rows without another copy or a read-back)
TENSOR_FIELDS = ("text_id", "label", "video_index", "label_mask") + scored.FIELDS
PLAIN_FIELDS = ("video", "video_len", "audio", "audio_len", "answer", "qtype")   # plain tensors, those the batch has (the
#                                                                 audio-only batch has no "video"): one staging buffer for all
HOST_FIELDS = ("video_start", "prefix_index", "vid", "text", "qid", scored.COUNT)   # stay on the host


def _tensor_items(batch: dict) -> List[Tuple[Tuple[str, Optional[str]], torch.Tensor]]:
    items = []
    for f in PLAIN_FIELDS:
        if f in batch and torch.is_tensor(batch[f]):
            items.append(((f, None), batch[f]))
    for f in TENSOR_FIELDS:
        if f in batch:
            for t, v in batch[f].items():
                if torch.is_tensor(v):
                    items.append(((f, t), v))
    return items


class PackedBatch:
    """What a DataLoader worker hands over when packing is pushed into the workers: ONE uint8 tensor (one
    shared-memory handle to receive instead of ~25) + the table of (field, task) -> (offset, shape, dtype) +
    the host-side fields."""
    __slots__ = ("blob", "meta", "host")

    def __init__(self, blob, meta, host):
        self.blob, self.meta, self.host = blob, meta, host


class _PackingCollate:
    """collate_fn wrapper: the reference-schema batch dict, flattened into a PackedBatch inside the worker."""

    def __init__(self, collate_fn):
        self.collate_fn = collate_fn

    def __call__(self, samples):
        batch = scored.annotate(self.collate_fn(samples))
        items = _tensor_items(batch)
        meta, off = {}, 0
        for key, v in items:
            meta[key] = (off, tuple(v.shape), v.dtype)
            off += (v.numel() * v.element_size() + _ALIGN - 1) // _ALIGN * _ALIGN
        blob = np.empty(max(off, _ALIGN), dtype=np.uint8)
        for key, v in items:
            o = meta[key][0]
            n = v.numel() * v.element_size()
            blob[o:o + n] = v.contiguous().numpy().reshape(-1).view(np.uint8)
        return PackedBatch(torch.from_numpy(blob), meta, {f: batch[f] for f in HOST_FIELDS if f in batch})


class _Slot:
    def __init__(self, nbytes: int, device: torch.device):
        cuda = device.type == "cuda"
        self.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=cuda)
        self.host_np = self.host.numpy()                          # same (pinned) memory
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device) if cuda else self.host
        self.copied = torch.cuda.Event() if cuda else None       # H2D of this slot finished
        self.released = torch.cuda.Event() if cuda else None     # compute stream is past the consumer step
        self.in_use = False


class DeviceBatchProducer:
    def __init__(self, loader: Iterable[dict], device, depth: int = 2, pack_in_workers: bool = True):
        """pack_in_workers: when `loader` is a torch DataLoader with worker processes, wrap its collate_fn so
        that the flattening into one buffer happens in the workers; the training process then spends ~0.2 ms
        of interpreter time per batch (one tensor to receive, one memcpy, one H2D) instead of ~3 ms."""
        self.loader = loader
        if pack_in_workers and getattr(loader, "num_workers", 0) > 0 and hasattr(loader, "collate_fn") \
                and not isinstance(loader.collate_fn, _PackingCollate):
            loader.collate_fn = _PackingCollate(loader.collate_fn)
        self.device = torch.device(device)
        self.depth = max(2, int(depth))
        self.cuda = self.device.type == "cuda"
        self.copy_stream = torch.cuda.Stream(device=self.device) if self.cuda else None
        self._slots: List[_Slot] = []
        self._layout = None            # [(key, dtype, per-sample shape, offset, max bytes)], total
        self._max_b = 0
        self.h2d_bytes = 0

    def __len__(self):
        return len(self.loader)

    # ------------------------------------------------------------------ layout
    def _make_layout(self, batch: dict):
        off, lay = 0, []
        self._max_b = int(batch["video"].shape[0]) if "video" in batch else \
            int(next(iter(batch["text_id"].values())).shape[0])
        for key, v in _tensor_items(batch):
            nbytes = v.numel() * v.element_size()
            lay.append((key, v.dtype, tuple(v.shape[1:]), off, nbytes))
            off += (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        self._layout = (lay, max(off, _ALIGN))
        self._slots = [_Slot(self._layout[1], self.device) for _ in range(self.depth)]

    def _pack(self, slot: _Slot, batch: dict) -> Tuple[dict, int]:
        """Copy the batch's tensors into the slot's staging buffer; -> (field -> (offset, shape, dtype), bytes used)."""
        lay, _ = self._layout
        have = dict(_tensor_items(batch))
        meta, used = {}, 0
        for key, dtype, tail, off, cap in lay:
            v = have[key]
            if v.dtype != dtype or tuple(v.shape[1:]) != tail or v.shape[0] > self._max_b:
                raise ValueError(f"batch field {key} changed layout: {tuple(v.shape)} {v.dtype}")
            n = v.numel() * v.element_size()
            # plain memcpy through numpy: a torch CPU op here would wake the whole intra-op thread pool
            # (128 threads on the MI355X host) for a few KB — measured 24 ms per batch against 0.1 ms
            src = v.contiguous().numpy().reshape(-1).view(np.uint8)
            np.copyto(slot.host_np[off:off + n], src)
            meta[key] = (off, tuple(v.shape), dtype)
            used = max(used, off + n)
        return meta, used

    def _views(self, slot: _Slot, meta: dict, batch: dict) -> dict:
        out = {f: batch[f] for f in HOST_FIELDS if f in batch}
        for (f, t), (off, shape, dtype) in meta.items():
            n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
            view = slot.dev[off:off + n].view(dtype).view(shape)
            if t is None:
                out[f] = view
            else:
                out.setdefault(f, {})[t] = view
        return out

    # ------------------------------------------------------------------ iteration
    def __iter__(self) -> Iterator[dict]:
        it = iter(self.loader)
        ready: "queue.Queue" = queue.Queue(maxsize=self.depth)
        free: "queue.Queue" = queue.Queue()
        stop = threading.Event()
        err: List[BaseException] = []
        handed_out = [False]

        def work():
            try:
                for batch in it:
                    if stop.is_set():
                        return
                    packed = isinstance(batch, PackedBatch)
                    if not packed:
                        batch = scored.annotate({k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()})
                    if self._layout is None:
                        if packed:
                            self._layout = ([], int(batch.blob.numel()))
                            self._slots = [_Slot(self._layout[1], self.device) for _ in range(self.depth)]
                        else:
                            self._make_layout(batch)
                    if not handed_out[0]:                 # once per epoch: every slot starts free
                        handed_out[0] = True
                        for s in self._slots:
                            free.put(s)
                    slot = free.get()
                    if stop.is_set():
                        return
                    if self.cuda:
                        slot.released.synchronize()       # the step that read this slot is done
                    if packed:
                        used = int(batch.blob.numel())
                        if used > self._layout[1]:
                            raise ValueError("a later batch is larger than the first one: staging slots too small")
                        np.copyto(slot.host_np[:used], batch.blob.numpy())
                        meta, batch = batch.meta, batch.host
                    else:
                        meta, used = self._pack(slot, batch)
                    if self.cuda:
                        with torch.cuda.stream(self.copy_stream):
                            slot.dev[:used].copy_(slot.host[:used], non_blocking=True)
                            slot.copied.record(self.copy_stream)
                    self.h2d_bytes += used
                    ready.put((slot, meta, batch))
            except BaseException as e:      # surfaced in the consumer
                err.append(e)
            finally:
                ready.put(None)

        th = threading.Thread(target=work, name="fvqa-batch-producer", daemon=True)
        th.start()
        prev: Optional[_Slot] = None
        try:
            while True:
                item = ready.get()
                if prev is not None:                      # the consumer has issued the step that used `prev`
                    if self.cuda:
                        prev.released.record(torch.cuda.current_stream(self.device))
                    free.put(prev)
                    prev = None
                if item is None:
                    break
                slot, meta, batch = item
                if self.cuda:
                    torch.cuda.current_stream(self.device).wait_event(slot.copied)
                prev = slot
                yield self._views(slot, meta, batch)
        finally:
            stop.set()
            free.put(None)
            while th.is_alive():
                try:
                    ready.get(timeout=0.05)
                except queue.Empty:
                    pass
            th.join()
        if err:
            raise err[0]
