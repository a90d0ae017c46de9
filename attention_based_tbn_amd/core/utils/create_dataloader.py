"""`create_dataloader(cfg, logger, modality, mode)` of the reference (`core/utils/create_dataloader.py:84-128`), returning a
`ClipLoader` over a device-side `Video_Dataset` instead of a `torch.utils.data.DataLoader`.

What differs from the DataLoader, on purpose:
  * a batch is made at once by `Video_Dataset.batch` (one decode and one transform launch per modality), not item by item
    and collated;
  * by default iteration is synchronous on the current stream: no background thread, no prefetch, no worker processes.
    The decode pool of `decode_jpegs` is the only host parallelism, so `cfg.num_workers` is accepted and ignored.
    `prefetch=N` (opt-in) makes the batches on ONE producer thread and a side stream beside the consumer's work, at most N
    finished batches ahead -- still no worker processes;
  * train order is `torch.randperm(N)`, drawn once per `__iter__` from the global torch generator.  That is a seeded,
    reproducible shuffle, but it is NOT pinned to the draw of `torch.utils.data.RandomSampler` (which seeds a generator
    of its own from the global one first): the same `torch.manual_seed` gives another order than the reference's loader.
The last, shorter batch is kept, as with the DataLoader's default `drop_last=False`.
`shard=(rank, world)` makes the loader one of `world`, one per rank of a data-parallel job: the same global batches, each
rank its contiguous share of every one (`ClipLoader`).
"""
import os
import queue
import threading
import weakref

import numpy as np
import torch

from ..dataset.dataset import Video_Dataset
from ..dataset.transform import get_transforms

_DEFAULT_RNG = type("_DefaultRng", (str,), {})("global")    # tells the default apart from an explicit rng="global"
_POLL = 0.1          # seconds: queue put / get time-out, after which the stop flag / the producer's life is looked at
_JOIN = 5.0          # seconds: how long close() waits for the producer


def _record_stream(x, stream):
    """`record_stream` on every device tensor of a nested (tuple / list / dict) batch; anything else passes"""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            x.record_stream(stream)
    elif isinstance(x, dict):
        for v in x.values():
            _record_stream(v, stream)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _record_stream(v, stream)


def _put(q, item, stop):
    """blocks while the queue is full, but never past the stop flag -> was the item queued?"""
    while not stop.is_set():
        try:
            q.put(item, timeout=_POLL)
            return True
        except queue.Full:
            pass
    return False


def share_of(n, rank, world):
    """rank `rank`'s share of a global batch of `n` clips: positions [floor(rank * n / world), floor((rank + 1) * n / world))"""
    return rank * n // world, (rank + 1) * n // world


class _Part(object):
    """one global batch of a pass as one rank sees it: its number in the pass, its dataset indices, and the positions
    [lo, hi) of them that are this rank's (`keep` None: the loader is not sharded and the whole batch is made)"""

    def __init__(self, no, indices, keep, world):
        self.no, self.indices, self.keep = no, indices, keep
        n = len(indices)
        self.share = (n if keep is None else len(keep), n, world)      # (n_r, n, W)

    def make(self, dataset, rng):
        """the batch, or None when this rank's share is empty (the draws of the whole global batch are made all the same)"""
        if self.keep is None:
            return dataset.batch(self.indices, rng=rng)
        return dataset.batch(self.indices, rng=rng, keep=self.keep)


def _produce(dataset, parts, rng, q, stop, stream, device):
    """the producer thread: `part.make(dataset, rng)` for every part, in order, on `stream`; each result is queued
    with its part and the event recorded behind it (an empty share is made for its draws and not queued).  Holds no
    reference to the iterator, so that one can be collected."""
    try:
        if stream is None:
            for part in parts:
                if stop.is_set():
                    return
                item = part.make(dataset, rng)
                if item is not None and not _put(q, ("batch", (part, item), None), stop):
                    return
        else:
            with torch.cuda.device(device), torch.cuda.stream(stream):
                for part in parts:
                    if stop.is_set():
                        return
                    item = part.make(dataset, rng)
                    if item is None:
                        continue
                    event = torch.cuda.Event()
                    event.record(stream)
                    if not _put(q, ("batch", (part, item), event), stop):
                        return
        _put(q, ("end", None, None), stop)
    except BaseException as e:      # delivered to the consumer at the __next__ that would have returned this batch
        _put(q, ("error", e, None), stop)


class _PrefetchIter(object):
    """one pass of a `ClipLoader(prefetch > 0)`: owns the producer thread, its queue and its stop flag"""

    def __init__(self, dataset, parts, rng, prefetch, stream, device, note):
        self._q = queue.Queue(maxsize=prefetch)
        self._stop = threading.Event()
        self._stream, self._done, self._note = stream, False, note
        self.thread = threading.Thread(target=_produce, name="ClipLoader-producer", daemon=True,
                                       args=(dataset, parts, rng, self._q, self._stop, stream, device))
        self.thread.start()

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        while True:
            try:
                kind, item, event = self._q.get(timeout=_POLL)
                break
            except queue.Empty:
                if self.thread.is_alive():
                    continue
                try:        # it may have queued its last word right before it ended
                    kind, item, event = self._q.get_nowait()
                    break
                except queue.Empty:
                    self.close()
                    raise RuntimeError("ClipLoader: the producer thread ended without a batch, an end mark or an error")
        if kind == "batch":
            part, item = item
            if event is not None:
                current = torch.cuda.current_stream(self._stream.device)
                current.wait_event(event)           # device-side wait: the host does not synchronise
                _record_stream(item, current)       # allocated on the loader stream, used (and freed) on this one
            self._note(part)
            return item
        self.close()
        if kind == "error":
            raise item
        raise StopIteration

    def close(self):
        """stops the producer between two batches and waits (bounded) for it; idempotent"""
        self._done = True
        self._stop.set()
        try:
            while True:         # a producer blocked in put() sees the flag at its next time-out; dropping is quicker
                self._q.get_nowait()
        except queue.Empty:
            pass
        if self.thread is not threading.current_thread():
            self.thread.join(_JOIN)
            if self._stream is not None and not self.thread.is_alive():
                # what the producer left on its stream (cached waveforms, ...) is ordered before later work here
                torch.cuda.current_stream(self._stream.device).wait_stream(self._stream)
                self._stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClipLoader(object):
    """iterable over the batches of a `Video_Dataset`: `len()` = ceil(N / batch_size), `.dataset`, `.batch_size`.

    `prefetch=0, rng="global"` (the default): `dataset.batch(part)` on the calling thread and the current stream, every
    random draw from the global NumPy / torch generators.

    `rng="private"`: `__iter__` draws, on the calling thread, the shuffle and then ONE seed from torch's global generator
    (`torch.randint(0, 2**31 - 1, (1,))`); the pass's plans draw from `np.random.RandomState(seed)`, handed to
    `dataset.batch(part, rng=)`.  A whole pass is then a function of the torch generator state at `__iter__`.

    `prefetch=N > 0` (implies and requires `rng="private"`): one daemon producer thread per `__iter__` makes the batches
    in order on a side stream of the loader's, never more than N finished batches plus the one in progress ahead of the
    consumer.  `__next__` makes the consumer's current stream wait for the batch's event and marks the batch's tensors
    as used on it (`record_stream`); the host does not synchronise.  The batches equal those of
    `ClipLoader(prefetch=0, rng="private")` under the same torch generator state.  An exception in the producer is
    raised at the `__next__` that would have returned its batch.  Leaving the loop early (`break`, an exception, the
    iterator closed or collected) or `close()` stops the producer within a bounded time.  One live iterator per
    loader: a second `__iter__` closes the first.

    While an iterator is live the dataset object must not be used by another thread: its waveform cache is mutated by
    the producer only.

    `shard=(rank, world)` (one loader per rank of a data-parallel job; `(0, 1)` and None are the unsharded loader).
    `batch_size` stays the GLOBAL batch and the global batches of a pass are exactly the unsharded loader's
    (`batches()`); of a global batch of n clips rank r makes positions [floor(r n / W), floor((r + 1) n / W)) and
    nothing else (`dataset.batch(part, rng=, keep=)`: every draw of the whole batch, the files of the kept clips only).
    `__iter__` has rank 0 draw the shuffle and the pass's NumPy seed from ITS torch generator and broadcast them -- one
    small collective per pass on the default process group (`process_group=`), issued on the calling thread, never on
    the producer's -- so a pass does not depend on the ranks' generators having stayed in step.  Implies and requires
    `rng="private"`.  Under one torch seed on rank 0 the ranks' batches, concatenated in rank order, are the batch of
    `ClipLoader(prefetch=0, rng="private")` at world 1 bit for bit, with and without `prefetch`.
    In train mode (`dataset.mode == "train"`) a global batch of fewer than W clips -- it would leave a rank without a
    backward to exchange gradients in -- is dropped on every rank and rank 0 logs one line; in val / test mode a rank
    whose share of a batch is empty makes that batch's draws and does not yield it.  `len()` stays the number of GLOBAL
    batches (without the dropped ones), so a rank may yield fewer.
    `broadcast=` replaces the collective: a callable that takes rank 0's int64 tensor `[seed, order...]` (zeros on the
    other ranks) and returns rank 0's (tests without a process group).

    For the batch most recently yielded the loop reads `loader.share = (n_r, n, W)` -- this rank's clips, the global
    batch's, the world size -- and `loader.batch_no`, the batch's number among the pass's global batches; both are set
    on the consumer's thread when the batch is handed out, and also by an unsharded loader (`(n, n, 1)`)."""

    def __init__(self, dataset, batch_size, shuffle=False, *, prefetch=0, rng=_DEFAULT_RNG, shard=None,
                 process_group=None, broadcast=None, logger=None):
        if batch_size < 1:
            raise ValueError(f"ClipLoader: batch_size {batch_size}")
        if int(prefetch) != prefetch or prefetch < 0:
            raise ValueError(f"ClipLoader: prefetch {prefetch!r} is not a count >= 0")
        if rng not in ("global", "private"):
            raise ValueError(f"ClipLoader: rng={rng!r} is not 'global' or 'private'")
        rank, world = 0, 1
        if shard is not None:
            try:
                rank, world = shard
                ok = int(rank) == rank and int(world) == world and world >= 1 and 0 <= rank < world
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"ClipLoader: shard={shard!r} is not (rank, world) with 0 <= rank < world")
        if prefetch > 0 or world > 1:
            if rng is not _DEFAULT_RNG and rng == "global":
                raise ValueError("ClipLoader: prefetch > 0 draws on another thread and shard=(r, W > 1) draws from a seed "
                                 "the ranks share; both need rng='private'")
            rng = "private"
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.prefetch, self.rng = int(prefetch), str(rng)
        self.rank, self.world = int(rank), int(world)
        self.process_group, self._broadcast, self._logger = process_group, broadcast, logger
        self.drops = self.world > 1 and getattr(dataset, "mode", None) == "train"
        self.share, self.batch_no = None, None
        self._stream, self._live = None, None

    def __len__(self):
        n = len(self.dataset)
        if not self.drops:
            return -(-n // self.batch_size)
        full, last = divmod(n, self.batch_size)
        return (full if self.batch_size >= self.world else 0) + (1 if last >= self.world else 0)

    def batches(self):
        """the index lists of one pass; with `shuffle` one `torch.randperm` draw from the global generator"""
        n = len(self.dataset)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        return [order[i:i + self.batch_size] for i in range(0, n, self.batch_size)]

    def _note(self, part):
        self.share, self.batch_no = part.share, part.no

    def _global_pass(self):
        for no, part in enumerate(self.batches()):
            item = self.dataset.batch(part)
            self._note(_Part(no, part, None, 1))
            yield item

    def _private_pass(self, parts, rng):
        for part in parts:
            item = part.make(self.dataset, rng)
            if item is not None:
                self._note(part)
                yield item

    def _exchange(self, packed):
        """rank 0's `[seed, order...]` on every rank: ONE broadcast over the process group"""
        if self._broadcast is not None:
            return self._broadcast(packed)
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError(f"ClipLoader: shard=({self.rank}, {self.world}) needs an initialised torch.distributed "
                               "process group (or broadcast=)")
        if dist.get_world_size(self.process_group) != self.world or dist.get_rank(self.process_group) != self.rank:
            raise RuntimeError(f"ClipLoader: shard=({self.rank}, {self.world}) is not this process's place in its group "
                               f"({dist.get_rank(self.process_group)}, {dist.get_world_size(self.process_group)})")
        src = dist.get_global_rank(self.process_group, 0) if self.process_group is not None else 0
        if dist.get_backend(self.process_group) == "nccl":
            device = torch.device(getattr(self.dataset, "device", "cuda"))
            packed = packed.to(device)
            dist.broadcast(packed, src, group=self.process_group)
            return packed.cpu()
        dist.broadcast(packed, src, group=self.process_group)
        return packed

    def _sharded_parts(self):
        """rank 0 draws the pass (the shuffle, then the seed: `__iter__`'s order) and broadcasts it -> (parts, seed)"""
        n = len(self.dataset)
        packed = torch.zeros(n + 1, dtype=torch.int64)
        if self.rank == 0:
            batches = self.batches()
            packed[0] = int(torch.randint(0, 2 ** 31 - 1, (1,)))
            packed[1:] = torch.tensor([i for part in batches for i in part], dtype=torch.int64)
        packed = self._exchange(packed).tolist()
        seed, order = packed[0], packed[1:]
        parts, dropped = [], 0
        for first in range(0, n, self.batch_size):
            indices = order[first:first + self.batch_size]
            if self.drops and len(indices) < self.world:
                dropped += 1
                continue
            lo, hi = share_of(len(indices), self.rank, self.world)
            parts.append(_Part(len(parts), indices, range(lo, hi), self.world))
        if dropped and self.rank == 0:
            import logging
            (self._logger or logging.getLogger(__name__)).info(
                f"ClipLoader: dropped {dropped} train batch(es) of fewer than {self.world} clips (one per rank is needed)")
        return parts, seed

    def _loader_stream(self):
        """(side stream, device), made on first use; (None, None) without CUDA"""
        if not torch.cuda.is_available():
            return None, None
        if self._stream is None:
            device = torch.device(getattr(self.dataset, "device", "cuda"))
            if device.type != "cuda":
                return None, None
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self._stream = torch.cuda.Stream(device=device)
        return self._stream, self._stream.device

    def __iter__(self):
        if self.rng == "global":
            return self._global_pass()
        self.close()
        if self.world > 1:
            parts, seed = self._sharded_parts()
        else:
            parts = [_Part(no, part, None, 1) for no, part in enumerate(self.batches())]
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
        rng = np.random.RandomState(seed)
        if self.prefetch == 0:
            return self._private_pass(parts, rng)
        stream, device = self._loader_stream()
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(device))    # e.g. waveforms cached by a synchronous pass
        live = _PrefetchIter(self.dataset, parts, rng, self.prefetch, stream, device, self._note)
        self._live = weakref.ref(live)      # weak: dropping the iterator (a `break`) collects it, which stops the producer
        return live

    def close(self):
        """stops the live prefetching iterator, if there is one (bounded wait); the loader can be iterated again"""
        live, self._live = (self._live() if self._live is not None else None), None
        if live is not None:
            live.close()


def create_dataloader(cfg, logger, modality, mode="test", device="cuda", *, prefetch=0, audio_load="host",
                      flow_load="host", shard=None, inflate="host"):
    """`shard=(rank, world)`: handed to `ClipLoader`; the mode's batch size stays the global batch.  The annotation file, video list and batch size per mode follow the reference (:86-120); val reads the TRAIN
    annotation file filtered by the val video list, as there.  A relative `vid_list` path is taken from the directory
    above the `core` package, like the reference's; an empty one keeps every video.  `prefetch` is handed to `ClipLoader`,
    `audio_load` ("host" / "device": who reads raw audio files) and `flow_load` ("host" / "device": who inflates the flow
    pickles of data.flow.read_flow_pickle) and `inflate` ("host" / "device": who inflates PNG frames, data.rgb.file_ext "png")
    to `Video_Dataset`."""
    logger.info(f"Creating {mode} Dataloader...")
    if mode == "train":
        vid_file, annotation_file, batch_size = cfg.train.vid_list, cfg.train.annotation_file, cfg.train.batch_size
    elif mode == "val":
        vid_file, annotation_file, batch_size = cfg.val.vid_list, cfg.train.annotation_file, cfg.val.batch_size
    elif mode == "test":
        vid_file, annotation_file, batch_size = cfg.test.vid_list, cfg.test.annotation_file, cfg.test.batch_size
    else:
        raise ValueError(f"create_dataloader: unknown mode {mode!r}")
    if not isinstance(annotation_file, str):
        raise TypeError(f"create_dataloader: {mode}.annotation_file is {annotation_file!r}; one loader reads one file "
                        "(the reference's test tool builds a dataset per file itself)")
    vid_list = None
    if vid_file:
        file_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        with open(os.path.join(file_dir, vid_file)) as f:
            vid_list = [x.strip() for x in f.readlines() if len(x.strip()) > 0]
    transforms = get_transforms(cfg, modality, mode, device=device, flow_length=2 * cfg.data.flow.win_length)
    dataset = Video_Dataset(cfg, vid_list, annotation_file, modality, transform=transforms, mode=mode, device=device,
                            audio_load=audio_load, flow_load=flow_load, inflate=inflate)
    loader = ClipLoader(dataset, batch_size, shuffle=(mode == "train"), prefetch=prefetch, shard=shard, logger=logger)
    logger.info("Done.")
    logger.info("----------------------------------------------------------")
    return loader
