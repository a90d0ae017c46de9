"""Data parallelism for the TBN hot path: one process per GPU, RCCL all-reduce over xGMI.

Replaces reference core/models/dataparallel.py:4-6 (single-process nn.DataParallel: per-step
parameter broadcast + scatter/gather + reduce to GPU 0).  Here every rank holds a replica, runs
the full forward/backward on its own shard of the clips (per-replica BatchNorm statistics, as
nn.DataParallel's chunks had) and gradients are averaged with one collective per LARGE parameter
tensor -- the backbones keep their parameters in a few flat tensors (~41 MB per backbone) -- plus ONE
for all small tensors (heads, biases, BN affine) packed into a flat buffer; a head tensor above 1 MB (the fusion Linear's
weight) travels on its own: five all-reduces per step with three modalities.
A backbone's flat gradient travels in buckets issued from INSIDE its backward as the engine reports slices final
(tbn_backbone_grads.bucket_cb: inception_5a..5b, then 4a..4e), i.e. under the rest of that backward and under the other
backbones' on their own HIP streams; the remaining prefixes and the packed small-tensor collective go at the end of
backward, behind every bucket (collectives execute in issue order).  No collective on the data path.

The collective SCHEDULE is the same on every rank by construction: the packed buffer always holds every
small trainable parameter in registration order (a missing gradient travels as zeros), and a large tensor is
reduced from inside its gradient hook only if the wrapped module does not declare it optional.  Parameters the
module lists in `maybe_unused_parameter_prefixes()` -- the audio backbone and the attention stack while
`data.audio.dropout > 0`: reference model.py:215-222 draws the drop decision per replica, so one rank may produce
those gradients while another does not -- are reduced at the end of backward in registration order, zero-filled
where absent, together with one presence flag each; a parameter no rank produced a gradient for gets `grad = None`
back, which is what the reference's optimiser sees when every nn.DataParallel replica dropped the audio feature.
The drop decision is a HOST draw made during forward: when the module also reports it (`optional_parameters_used()`),
the ranks exchange it right after forward -- a 1-element all-reduce on a side stream, read back through a pinned buffer
and an event, never through the compute stream -- so that every rank knows BEFORE backward whether all, some or none of
the replicas kept the branch: all -> the optional tensors are reduced from their gradient hooks like any other (the
~41 MB audio backbone overlaps the other backbones' backward instead of being exposed at the end), none -> they are
skipped and come back as `grad = None` without any end-of-step host read, some -> the zero-filled end-of-backward path.

`DataParallel(model)` keeps the reference surface: `.module`, `forward`, `get_loss(...)`,
`state_dict()` of the wrapped model under the `module.` prefix.
"""
import torch
import torch.distributed as dist
import torch.nn as nn


class PlanSync:
    """moves rank 0's tuned engine plans to every replica (reference nn.DataParallel replicas are identical by
    construction, core/models/model_builder.py:73-75).  Called from inside the first forward of a new (shape, mode) on
    every rank alike -- same shapes on every rank, so the broadcasts match up."""

    def __init__(self, process_group=None, src=0):
        self.group, self.src = process_group, src

    def is_source(self):
        return dist.get_rank(self.group) == self.src

    def check(self, key, device):
        """every rank must be about to exchange the plan of the SAME problem and mode: all-gather the key and raise on every
        rank alike when they differ (a last batch whose frame count differs between ranks, a rank in eval while the others
        train) -- the alternative is a broadcast that pairs a blob with the wrong plan, or ranks waiting in different
        collectives.  What this cannot catch is a rank that never gets here (a forward run by a subset of the ranks): such
        callers set `module.plan_sync = None` first (BNInception.plan_sync)."""
        keys = [None] * dist.get_world_size(self.group)
        dist.all_gather_object(keys, tuple(int(v) for v in key), group=self.group)
        if any(k != keys[0] for k in keys):
            raise RuntimeError("PlanSync: the ranks are exchanging engine plans for different problems "
                               "(in_channels, frames, H, W, training) = %s; every rank must run the same shapes in the same "
                               "mode, or bypass the exchange with plan_sync = None" % (keys,))

    def broadcast(self, blob, device):
        t = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        if dist.get_backend(self.group) == "nccl":
            t = t.to(device)
        dist.broadcast(t, dist.get_global_rank(self.group, self.src) if self.group is not None else self.src,
                       group=self.group)
        return bytes(t.cpu().numpy().tobytes())


class DataParallel(nn.Module):
    SMALL = 1 << 18   # elements: gradients below 1 MB travel together in one flat buffer (one collective)

    def __init__(self, module, device_ids=None, process_group=None, broadcast_parameters=True, overlap=True,
                 force_sync=False):
        """`force_sync`: register the gradient hooks and run every collective even when the group has ONE rank (the
        default wraps a lone rank as a pass-through) -- puts the real hook -> all_reduce(async_op) -> queue_callback ->
        work.wait() path under RCCL's stream semantics on a single GPU (tests/test_dp_gpu.py)."""
        super().__init__()
        self.module = module
        self.device_ids = device_ids
        self.process_group = process_group
        self.overlap = overlap          # False: every collective at the end of backward (diagnostic)
        self.time_sync = False          # bench: bracket finish_gradient_sync with events (exposed all-reduce time)
        self._sync_events = []
        self._pending = []              # (param, reduced view of its .grad, work) of the collectives issued from gradient hooks
        self._bucketed = {}             # id(param) -> lowest element already exchanged from inside its backward (buckets)
        self.bucket_log = []            # (parameter numel, lo, hi) of every bucket collective, in issue order (tests, bench)
        self._fired = set()             # ids of the parameters whose gradient hook ran in this backward
        self._callback_queued = False
        self._hooks = []
        self._sync = True               # False inside no_sync(): gradients stay local (accumulation steps, tests)
        self.grad_weight = None         # see weigh_next_backward(): factor on this rank's gradients in the NEXT exchange
        self._presence = None           # ("pending", event, pinned host tensor) | ("count", n): see _exchange_presence
        self._side_stream = None
        self._host_flag = None
        self._forwards_pending = 0      # training forwards since the last synchronised backward (see forward())
        self._unsynced = False          # a backward under no_sync() has left LOCAL sums in .grad since the last exchange
        self.world_size = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        if force_sync and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("DataParallel(force_sync=True) needs an initialised process group")
        self.active = self.world_size > 1 or force_sync
        if self.active:
            if broadcast_parameters:
                self.broadcast_parameters()
            if self.world_size > 1:
                sync = PlanSync(process_group)
                for m in self.module.modules():
                    if hasattr(m, "plan_sync"):
                        m.plan_sync = sync       # BNInception: autotune on rank 0 only, choices broadcast
            for m in self.module.modules():
                if hasattr(m, "grad_bucket_fn"):
                    m.grad_bucket_fn = self._on_grad_bucket     # BNInception: slices of the flat gradient as they become final
            for p in self.module.parameters():
                if p.requires_grad:
                    self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad_ready))

    def broadcast_parameters(self, src=0):
        """rank `src`'s parameters and buffers become everyone's (once, at wrap time): one broadcast per dtype over a
        flat buffer -- the same coalescing the gradient all-reduce uses -- instead of one per tensor (1464 of them)"""
        self._broadcast_flat(list(self.module.parameters()) + list(self.module.buffers()), src)

    def broadcast_buffers(self, src=0):
        """rank `src`'s buffers (the BatchNorm running statistics) become everyone's, by the same flat broadcast: the
        reference's nn.DataParallel keeps replica 0's running statistics as the model's, so the epoch loops call this
        before each validation and before the checkpoint is written.  No-op for a lone rank."""
        if self.world_size > 1:
            self._broadcast_flat(list(self.module.buffers()), src)

    def _broadcast_flat(self, tensors, src):
        with torch.no_grad():
            by_dtype = {}
            for t in tensors:
                by_dtype.setdefault((t.dtype, t.device), []).append(t)
            for group in by_dtype.values():
                flat = torch.cat([t.reshape(-1) for t in group])
                dist.broadcast(flat, src, group=self.process_group)
                off = 0
                for t in group:
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()

    def _reduce_op(self):
        avg = dist.get_backend(self.process_group) == "nccl"
        return avg, (dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM)

    def _optional_ids(self):
        """parameters that may legitimately get no gradient on some ranks in this step (declared by the module)"""
        fn = getattr(self.module, "maybe_unused_parameter_prefixes", None)
        prefixes = tuple(fn()) if fn is not None else ()
        if not prefixes:
            return set()
        return {id(p) for n, p in self.module.named_parameters() if p.requires_grad and n.startswith(prefixes)}

    def no_sync(self):
        """context manager: backward passes inside it leave the gradients un-reduced (as torch DDP's `no_sync`)"""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            old, self._sync = self._sync, False
            try:
                yield
            finally:
                self._sync = old
        return ctx()

    def weigh_next_backward(self, weight):
        """the NEXT synchronised backward exchanges `weight` times this rank's gradients: with weight_r = n_r W / n the
        average over the ranks is sum_r (n_r / n) g_r, the gradient of a mean over a global batch of n clips of which
        this rank holds n_r (`TrainStep(share=)`).  Every gradient is multiplied ONCE, finished, right before its
        collective is issued (gradient hook, bucket, end-of-backward tensors and the packed buffer alike) -- the backward
        pass itself runs exactly as without a weight, so g_r keeps its bits.  Only right when `.grad` holds nothing
        before that backward (every tensor is then what this backward produced); a caller that accumulates scales its
        loss instead.  None clears it; the exchange clears it too."""
        self.grad_weight = None if weight is None else float(weight)

    def _weigh(self, t):
        if self.grad_weight is not None and t.numel():
            t.mul_(self.grad_weight)

    def _exchange_presence(self):
        """after a training forward: how many replicas used the optional parameters in this step (the module's
        host-side draw).  Issued on a side stream so that neither the collective nor the read-back waits for the
        forward kernels queued on the compute stream."""
        self._presence = None
        fn = getattr(self.module, "optional_parameters_used", None)
        if fn is None or not self._optional_ids():
            return
        used = 1.0 if fn() else 0.0
        dev = next(self.module.parameters()).device
        if dev.type == "cuda":
            if self._side_stream is None:
                self._side_stream = torch.cuda.Stream(device=dev)
                self._host_flag = torch.zeros(1, dtype=torch.float32).pin_memory()
            with torch.cuda.stream(self._side_stream):
                t = torch.tensor([used], dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.process_group, async_op=True).wait()
                self._host_flag.copy_(t, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._side_stream)
            self._presence = ("pending", ev, t)      # `t` kept alive until the copy has run
        else:
            t = torch.tensor([used])
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.process_group)
            self._presence = ("count", int(round(float(t.item()))))

    def _presence_count(self):
        """number of replicas that used the optional parameters in this step, or None when the module does not report it"""
        if self._presence is None:
            return None
        if self._presence[0] == "pending":
            self._presence[1].synchronize()          # the side stream's copy: microseconds, not the step's kernels
            self._presence = ("count", int(round(float(self._host_flag.item()))))
        return self._presence[1]

    def _on_grad_ready(self, p):
        """post-accumulate-grad hook.  A large (flat backbone) gradient is all-reduced right here: the hook
        runs inside the AccumulateGrad node, whose stream the autograd engine has already made wait for the
        producing backbone's side stream (the stream semantics torch's own DDP reducer relies on), and the
        process group orders its collective after the current stream -- so the transfer starts when THAT
        backbone's backward has finished on the GPU, under the backward of the others.  Hooks fire in the
        same (reverse-forward) order on every rank and only for parameters every rank produces (optional ones
        wait for the end), so the collectives match up.  Small tensors are only remembered; one callback at
        the end of backward packs and reduces them and waits for everything."""
        if not self._sync:
            self._unsynced = True        # accumulation step: what sits in .grad now differs from rank to rank
            return
        self._begin_backward()
        self._fired.add(id(p))
        if self.overlap and p.grad is not None and p.grad.numel() >= self.SMALL and id(p) not in self._optional:
            _, op = self._reduce_op()
            if id(p) in self._bucketed:
                # buckets of this tensor were exchanged from inside its backward: only the prefix below them is left (the
                # stem / 3a..3c weights of a backbone, ~10 %).  It is final only when this backbone's WHOLE backward has run
                # on the GPU -- about the end of the step, the three backward passes end together -- and collectives
                # execute in issue order: issued here, it would hold up the buckets of the backbones whose backward is
                # enqueued AFTER this one (ready long before) until then.  So the prefix waits for the end of backward.
                self._pending.append((p, p.grad.view(-1)[:self._bucketed[id(p)]], None))
            else:
                self._weigh(p.grad)
                self._pending.append((p, p.grad, dist.all_reduce(p.grad, op=op, group=self.process_group, async_op=True)))

    def _begin_backward(self):
        """first gradient event of a synchronised backward (a hook or a bucket): fix what is optional in THIS step and
        queue the end-of-backward callback"""
        if self._callback_queued:
            return
        self._callback_queued = True
        self._optional = self._optional_ids()
        self._optional_all = set(self._optional)
        self._count = self._presence_count() if self._optional else None
        if self._count == self.world_size:
            self._optional = set()       # every replica produced them: ordinary, hook-overlapped reduction
        torch.autograd.Variable._execution_engine.queue_callback(self.finish_gradient_sync)

    def _on_grad_bucket(self, p, fresh, lo, hi):
        """called from INSIDE a backbone's backward (BNInception.grad_bucket_fn, engine callback
        tbn_backbone_grads.bucket_cb) when elements [lo, hi) of the gradient `fresh` of parameter `p` are final in stream
        order: their all-reduce starts now and runs under the rest of that backward -- the reference's nn.DataParallel
        reduces per backward too (core/models/model_builder.py:73-75), SURVEY 8e asks for buckets "launched as backward
        produces them".  Only while the result is going to BE the gradient (p.grad is None: nothing accumulated locally,
        which is the same on every rank) and the parameter is reduced from hooks at all; otherwise the whole tensor takes the
        ordinary path.  Buckets arrive top-down (hi of one = lo of the previous), on every rank alike.
        Returns a waiter the backward calls before it hands `fresh` to autograd (stream-level under RCCL)."""
        if not (self.active and self._sync and self.overlap) or p.grad is not None or hi - lo < self.SMALL:
            return None
        self._begin_backward()
        if id(p) in self._optional:
            return None
        if self._bucketed.get(id(p), fresh.numel()) != hi:
            return None                  # not the next slice down: leave the rest to the hook
        avg, op = self._reduce_op()
        view = fresh.view(-1)[lo:hi]
        self._weigh(view)
        work = dist.all_reduce(view, op=op, group=self.process_group, async_op=True)
        self._bucketed[id(p)] = lo
        self.bucket_log.append((fresh.numel(), lo, hi))
        if len(self.bucket_log) > 64:
            del self.bucket_log[:-64]

        def wait():
            work.wait()
            if not avg:
                view.div_(self.world_size)
        return wait

    def finish_gradient_sync(self):
        """average every gradient produced by this backward across ranks (RCCL all-reduce): one collective per
        large (flat backbone) tensor -- already in flight when `overlap` -- and ONE for all the small head /
        bias / BN tensors together.  Runs as the autograd engine's final callback, before backward() returns."""
        self._check_peer_flag()
        avg, op = self._reduce_op()
        ev0 = None
        if self.time_sync and torch.cuda.is_available():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        optional = getattr(self, "_optional", set())
        count = getattr(self, "_count", None)
        # "nobody": known before backward that no replica used the optional parameters in THIS iteration -- their
        # reduction is skipped and .grad stays as it is (None after zero_grad, or what earlier SYNCHRONISED iterations of an
        # accumulation window left there: identical on every rank already; reference core/tools/train.py:71-94 keeps
        # accumulating into .grad and steps on it).  Not when a no_sync() backward has left rank-local sums behind: those
        # still have to be exchanged, whoever produced them (round-5 advisor)
        nobody = count == 0 and not self._unsynced
        mismatch = False
        if count is not None:
            # the exchanged draw must describe THIS backward: a rank whose optional parameters fired although "nobody"
            # kept them (or did not although "all" did) would issue a different collective schedule than its peers and
            # hang the job inside RCCL -- fail loudly instead, and (round-4 advisor) fail on EVERY rank:
            produced = [id(p) in self._fired and p.grad is not None
                        for p in self.module.parameters() if id(p) in getattr(self, "_optional_all", set())]
            if count == self.world_size and not all(produced):
                # the peers reduced the optional tensors from their gradient hooks, in hook order; this rank's hooks never
                # fired, so it cannot join those collectives in order any more.  Drain what is in flight (nothing may
                # still be writing p.grad when the exception unwinds), then take the communicator down so that the peers'
                # collectives fail now instead of at the RCCL timeout (torch implements abort for the nccl backend only)
                self._drain_and_reset()
                self._abort_group()
                raise RuntimeError(self._MISMATCH % (count, self.world_size))
            # "nobody" was exchanged but this rank produced them: the peers' schedule (optional tensors skipped) is one
            # this rank can follow exactly -- it does, with a flag in the packed buffer, and all ranks raise together
            mismatch = nobody and any(produced)
        in_flight = {id(p) for p, _, _ in self._pending}
        params = [p for p in self.module.parameters() if p.requires_grad]      # registration order: rank independent
        present = {}
        for p in params:
            if id(p) in optional:
                # whatever this rank holds travels: the gradient of this backward, and / or what earlier iterations of an
                # accumulation window accumulated (a rank that dropped the branch NOW still contributes its accumulated
                # part -- under per-iteration synchronisation that part is the same on every rank and averages to itself)
                present[id(p)] = p.grad is not None
                if not present[id(p)] and not nobody:
                    p.grad = torch.zeros_like(p)         # nothing here: contributes zeros, same schedule
        # a non-optional parameter without a gradient is skipped -- on every rank alike (same contract as torch DDP
        # with find_unused_parameters=False); small ones still travel (as zeros) so that the packed size is fixed
        # ("nobody": the optional tensors are skipped -- also on a rank whose backward produced them against the draw)
        late_large = [p for p in params if p.numel() >= self.SMALL and id(p) not in in_flight and p.grad is not None
                      and not (nobody and id(p) in optional)]
        small = [p for p in params if p.numel() < self.SMALL]
        works = [w for _, _, w in self._pending if w is not None]
        for p in late_large:
            self._weigh(p.grad)
        works += [dist.all_reduce(p.grad, op=op, group=self.process_group, async_op=True) for p in late_large]
        # the prefixes of the bucketed tensors (see _on_grad_ready): now, behind every bucket of every backbone
        for i, (p, view, w) in enumerate(self._pending):
            if w is None and view.numel():
                self._weigh(view)
                w = dist.all_reduce(view, op=op, group=self.process_group, async_op=True)
                self._pending[i] = (p, view, w)
                works.append(w)
        opt_list = [p for p in params if id(p) in optional]
        flat = None
        if small or opt_list:
            ref = (small or opt_list)[0]
            pieces = [(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in small]
            flags = [1.0 if present[id(p)] else 0.0 for p in opt_list]
            if count is not None:
                flags.append(1.0 if mismatch else 0.0)       # some rank's gradients contradict the exchanged draw
            flags = torch.tensor(flags, dtype=ref.dtype, device=ref.device)
            flat = torch.cat(pieces + [flags])
            self._weigh(flat[:flat.numel() - flags.numel()])       # the gradients, not the presence flags
            works.append(dist.all_reduce(flat, op=op, group=self.process_group, async_op=True))
        for work in works:
            work.wait()          # stream-level wait on RCCL; host-blocking only on gloo
        if not avg:
            for _, view, w in self._pending:
                if w is not None:
                    view.div_(self.world_size)
            for p in late_large:
                p.grad.div_(self.world_size)
            if flat is not None:
                flat.div_(self.world_size)
        if flat is not None:
            off = 0
            for p in small:
                if p.grad is not None:
                    p.grad.copy_(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
            if opt_list:
                if count is None:
                    # the module does not report its draw: one host read per step tells which tensors nobody produced
                    anyone = (flat[off:off + len(opt_list)].cpu() > 0).tolist()
                elif nobody:
                    anyone = [True] * len(opt_list)            # skipped above: .grad is left exactly as it was
                elif count == 0 or self._unsynced:
                    # rank-local accumulated sums were exchanged; which tensors NO rank held anything for is only in the flags
                    anyone = (flat[off:off + len(opt_list)].cpu() > 0).tolist()
                else:
                    anyone = [True] * len(opt_list)            # some replica produced them in this very backward
                for p, a in zip(opt_list, anyone):
                    if not a:
                        p.grad = None                      # no replica holds a gradient for it: the optimiser skips it
            if count is not None:
                self._stash_peer_flag(flat[-1:])           # read at the NEXT forward / backward: no end-of-step host sync
        if ev0 is not None:
            ev1.record()
            self._sync_events.append((ev0, ev1))
        self._pending = []
        self._bucketed = {}
        self._fired = set()
        self._callback_queued = False
        self._presence = None
        self._count = None
        self._forwards_pending = 0
        self._unsynced = False
        self.grad_weight = None
        if mismatch:
            # this rank followed the peers' schedule, i.e. its optional gradients were NOT reduced: drop them (the peers
            # hold None as well, so the replicas stay identical) and fail here; the peers fail at their next forward /
            # backward, when they read the flag that travelled in the packed buffer
            for p in self.module.parameters():
                if id(p) in getattr(self, "_optional_all", set()):
                    p.grad = None
            self._peer_flag = None
            raise RuntimeError(self._MISMATCH % (count, self.world_size))

    def _stash_peer_flag(self, flag):
        if flag.is_cuda:
            host = torch.zeros(1, dtype=flag.dtype).pin_memory()
            host.copy_(flag, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._peer_flag = (ev, host, flag)          # `flag` kept alive until the copy has run
        else:
            self._peer_flag = (None, flag.clone(), None)

    def _check_peer_flag(self):
        """raises when some rank reported, in the previous synchronised backward, gradients that contradict the exchanged
        draw (that rank raised right away; this one learns it from the flag in the packed buffer -- checked one call
        later so that no step ends in a host-device synchronisation)"""
        pf, self._peer_flag = getattr(self, "_peer_flag", None), None
        if pf is None:
            return
        if pf[0] is not None:
            pf[0].synchronize()
        if float(pf[1][0]) > 0:
            self._drain_and_reset()
            raise RuntimeError(self._MISMATCH % (-1, self.world_size) + " (reported by a peer rank in the previous step)")

    _MISMATCH = ("DataParallel: the optional-parameter draw exchanged after forward (%d of %d replicas) does not match the "
                 "gradients this backward produced on some rank; one forward per backward is assumed when the module "
                 "reports its draw")

    def _drain_and_reset(self):
        """error paths: wait for every collective already issued on p.grad (an exception must not leave RCCL writing
        into gradients the caller may free or reuse), then clear the per-step state"""
        for _, _, work in self._pending:
            try:
                if work is not None:
                    work.wait()
            except Exception:      # the collective itself failed: nothing left to drain
                pass
        self._pending, self._fired, self._callback_queued, self._presence, self._count = [], set(), False, None, None
        self._bucketed = {}
        self._forwards_pending = 0
        self.grad_weight = None

    def _abort_group(self):
        try:
            if dist.get_backend(self.process_group) == "nccl":
                from torch.distributed.distributed_c10d import _abort_process_group
                _abort_process_group(self.process_group)
        except Exception:          # best effort: the RuntimeError raised next is the message that matters
            pass

    def exposed_sync_ms(self):
        """mean GPU time the compute stream spent inside finish_gradient_sync (the all-reduce tail that backward did
        not hide + the small-tensor packing) over the steps recorded with `time_sync`; call after a device sync"""
        if not self._sync_events:
            return None
        ms = [a.elapsed_time(b) for a, b in self._sync_events]
        self._sync_events = []
        return sum(ms) / len(ms)

    def forward(self, *args, **kwargs):
        if self.active:
            self._check_peer_flag()
        out = self.module(*args, **kwargs)
        if self.active and self._sync and self.module.training and torch.is_grad_enabled():
            # the module's draw is per forward, the exchange describes ONE forward: when a second training forward
            # arrives before the backward of the first (two forwards feeding one backward, or a forward whose loss was
            # never back-propagated), the count no longer says which gradients the coming backward produces -> drop it
            # and let that backward take the presence-flag path (rank-independent schedule, one host read at its end).
            # Every rank runs the same number of forwards, so they all take the same branch.
            if self._forwards_pending == 0:
                self._exchange_presence()
            else:
                self._presence = None
            self._forwards_pending += 1
        return out

    def get_loss(self, criterion, target, preds, epoch=0):
        return self.module.get_loss(criterion, target, preds, epoch)

    @property
    def conv_math(self):
        return self.module.conv_math

    @conv_math.setter
    def conv_math(self, value):
        self.module.conv_math = value

    @property
    def conv_math_layers(self):
        return self.module.conv_math_layers

    @conv_math_layers.setter
    def conv_math_layers(self, value):
        self.module.conv_math_layers = value
