"""`ClipLoader(shard=(rank, world))` on a stub dataset that records its calls, `Video_Dataset.plan(keep=)` on the synthetic
dataset, and the loss scale of `TrainStep` on a two-term model.  No GPU, no process group: the loaders' one collective
per pass is replaced by `broadcast=`."""
import itertools
import threading

import numpy as np
import pytest
import torch

from tests import clip_loader_util as U

MODALITY = ["RGB", "Flow", "Audio"]


class Stub(object):
    """`batch(indices, rng=None, keep=None)`: ONE draw per call, whatever `keep` says -> (kept indices, the draw), or None
    for an empty `keep`; remembers (indices, keep, thread) of every call"""

    def __init__(self, n, mode):
        self.n, self.mode, self.calls = n, mode, []

    def __len__(self):
        return self.n

    def batch(self, indices, rng=None, **kw):
        draw = -1 if rng is None else int(rng.randint(1 << 30))
        keep = kw.get("keep")
        self.calls.append((list(indices), None if "keep" not in kw else list(keep), threading.current_thread()))
        if "keep" not in kw:
            return list(indices), draw
        if len(keep) == 0:
            return None
        return [indices[k] for k in keep], draw


def _pass(stub, B, W, seed, prefetch=0):
    """one pass of every rank's loader; rank 0 under torch seed `seed`, the others under seeds of their own
    -> per rank [(batch_no, share, item)], the loaders"""
    from attention_based_tbn_amd.core.utils import ClipLoader
    sent = {}

    def rank0(packed):
        sent["packed"] = packed.clone()
        return packed

    def other(packed):
        assert int(packed.abs().sum()) == 0             # a rank other than 0 draws nothing
        return sent["packed"].clone()

    out, loaders = [], []
    for r in range(W):
        torch.manual_seed(seed if r == 0 else 1000 + r)
        before = torch.get_rng_state()
        loader = ClipLoader(stub, B, shuffle=(stub.mode == "train"), prefetch=prefetch, shard=(r, W), rng="private",
                            broadcast=rank0 if r == 0 else other)
        got = []
        for item in loader:
            got.append((loader.batch_no, loader.share, item))
        if r > 0 and W > 1:
            assert torch.equal(before, torch.get_rng_state())
        out.append(got)
        loaders.append(loader)
    return out, loaders


@pytest.mark.parametrize("mode", ["train", "val"])
@pytest.mark.parametrize("N,B,W", list(itertools.product(range(1, 10), range(1, 5), range(1, 4))))
def test_shares_concatenate_to_the_global_batches(N, B, W, mode):
    from attention_based_tbn_amd.core.utils import ClipLoader
    seed = 7 * N + B
    torch.manual_seed(seed)
    twin = list(ClipLoader(Stub(N, mode), B, shuffle=(mode == "train"), rng="private"))
    assert len(twin) == -(-N // B)
    if mode == "train" and W > 1:
        twin = [t for t in twin if len(t[0]) >= W]       # dropped on every rank alike; only ever the tail of the pass
    stub = Stub(N, mode)
    ranks, loaders = _pass(stub, B, W, seed)
    assert all(len(loader) == len(twin) for loader in loaders)
    for no, (want, draw) in enumerate(twin):
        parts = [[g for g in got if g[0] == no] for got in ranks]
        assert all(len(p) <= 1 for p in parts)
        joined = [i for p in parts for g in p for i in g[2][0]]
        assert joined == want, (no, parts)
        n = len(want)
        for r, p in enumerate(parts):
            n_r = (r + 1) * n // W - r * n // W
            assert (len(p) == 1) == (n_r > 0)
            if p:
                assert p[0][1] == (n_r, n, W) and p[0][2][1] == draw and len(p[0][2][0]) == n_r
    # nothing but the twin's batches was yielded, in order
    for got in ranks:
        assert [g[0] for g in got] == sorted(g[0] for g in got) and all(g[0] < len(twin) for g in got)
    if W > 1:
        # every rank called the dataset once per kept global batch, empty shares included (the draws stay in step)
        per_rank = len(stub.calls) // W
        assert per_rank == len(twin) and len(stub.calls) == W * per_rank
        assert all(keep is not None for _, keep, _ in stub.calls)
    else:
        assert all(keep is None for _, keep, _ in stub.calls)      # (0, 1): the unsharded call, no keep= at all


@pytest.mark.parametrize("N,B,W", [(5, 2, 2), (3, 3, 2), (7, 3, 3)])
def test_prefetched_shares_equal_the_synchronous_ones(N, B, W):
    for mode in ("train", "val"):
        a, _ = _pass(Stub(N, mode), B, W, 11)
        stub = Stub(N, mode)
        b, _ = _pass(stub, B, W, 11, prefetch=2)
        assert a == b
        assert all(t.name == "ClipLoader-producer" for _, _, t in stub.calls)
    assert not [t for t in threading.enumerate() if t.name == "ClipLoader-producer" and t.is_alive()]


def test_shard_0_1_is_the_unsharded_loader():
    from attention_based_tbn_amd.core.utils import ClipLoader
    for kw in ({}, {"rng": "private"}, {"prefetch": 2}):
        got = []
        for shard in (None, (0, 1)):
            torch.manual_seed(3)
            np.random.seed(3)
            stub = Stub(5, "train")
            loader = ClipLoader(stub, 2, shuffle=True, shard=shard, **kw)
            items = []
            for item in loader:
                items.append((item, loader.share, loader.batch_no))
            got.append((items, [c[:2] for c in stub.calls], loader.rng, len(loader)))
        assert got[0] == got[1]
        assert [s for _, s, _ in got[0][0]] == [(2, 2, 1), (2, 2, 1), (1, 1, 1)]
        assert [no for _, _, no in got[0][0]] == [0, 1, 2]
    assert ClipLoader(Stub(5, "train"), 2, shard=(0, 1)).rng == "global"


def test_len_counts_global_batches_without_the_dropped_ones():
    from attention_based_tbn_amd.core.utils import ClipLoader
    assert len(ClipLoader(Stub(7, "train"), 3, shard=(1, 2))) == 2         # 3 + 3 + (1 < 2: dropped)
    assert len(ClipLoader(Stub(7, "val"), 3, shard=(1, 2))) == 3
    assert len(ClipLoader(Stub(8, "train"), 3, shard=(1, 2))) == 3         # the last batch has 2 clips: kept
    assert len(ClipLoader(Stub(8, "train"), 2, shard=(0, 3))) == 0         # no batch feeds three ranks
    assert len(ClipLoader(Stub(7, "train"), 3, shard=(0, 1))) == 3


def test_dropped_batch_is_logged_once_by_rank_0():
    import logging
    from attention_based_tbn_amd.core.utils import ClipLoader
    records = []
    log = logging.getLogger("shard_loader_test")
    handler = logging.Handler()
    handler.emit = records.append
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    try:
        sent = {}
        for r in range(2):
            loader = ClipLoader(Stub(3, "train"), 2, shuffle=True, shard=(r, 2), logger=log,
                                broadcast=(lambda p: sent.setdefault("p", p)) if r == 0 else (lambda p: sent["p"]))
            assert len(list(loader)) == 1
            assert len(records) == 1 and "dropped 1 train batch" in records[0].getMessage()
    finally:
        log.removeHandler(handler)


@pytest.mark.parametrize("shard", [(2, 2), (-1, 2), (0, 0), (0.5, 2), (1,), 3, ("a", "b"), (0, 1, 2)])
def test_bad_shards_raise(shard):
    from attention_based_tbn_amd.core.utils import ClipLoader
    with pytest.raises(ValueError):
        ClipLoader(Stub(4, "val"), 2, shard=shard)


def test_sharding_needs_the_private_rng_and_a_group():
    from attention_based_tbn_amd.core.utils import ClipLoader
    with pytest.raises(ValueError):
        ClipLoader(Stub(4, "val"), 2, shard=(0, 2), rng="global")
    assert ClipLoader(Stub(4, "val"), 2, shard=(0, 2)).rng == "private"
    with pytest.raises(RuntimeError):
        iter(ClipLoader(Stub(4, "val"), 2, shard=(0, 2)))          # no process group and no broadcast=


def test_share_of_is_a_partition():
    from attention_based_tbn_amd.core.utils.create_dataloader import share_of
    for n in range(0, 12):
        for W in range(1, 5):
            cuts = [share_of(n, r, W) for r in range(W)]
            assert cuts[0][0] == 0 and cuts[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            assert all(hi - lo in (n // W, n // W + 1) for lo, hi in cuts)


@pytest.mark.parametrize("sampling", ["sync", "async"])
def test_plan_keep_makes_every_draw_and_reads_one_header_per_foreign_modality(tmp_path, sampling, monkeypatch):
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import dataset as D
    cfg = load_config(U.write_dataset(tmp_path) + ["data.sampling=" + sampling])
    ds = U.make_dataset(cfg, MODALITY, "train")
    idx = [2, 0, 1]
    whole = ds.plan(idx, rng=np.random.RandomState(5))
    reads, headers = [], []
    real_read, real_size = D.FrameReader._read, D.jpeg_frame_size
    monkeypatch.setattr(D.FrameReader, "_read", staticmethod(lambda p: (reads.append(p), real_read(p))[1]))
    monkeypatch.setattr(D, "jpeg_frame_size", lambda p: (headers.append(p), real_size(p))[1])
    for keep in ([1], [], [0, 2], [0, 1, 2]):
        twin = np.random.RandomState(5)
        ds.plan(idx, rng=twin)
        del reads[:], headers[:]
        rng = np.random.RandomState(5)
        part = ds.plan(idx, rng=rng, keep=keep)
        assert np.array_equal(rng.get_state()[1], twin.get_state()[1]) and rng.get_state()[2] == twin.get_state()[2]
        assert [c.kept for c in part] == [i in keep for i in range(3)]
        for a, b in zip(whole, part):
            for m in MODALITY:
                assert np.array_equal(a.indices[m], b.indices[m]), m
            for m in ("RGB", "Flow"):
                ga, gb = a.visual[m].geo, b.visual[m].geo
                assert (ga.box, ga.resized, ga.crop, ga.flip) == (gb.box, gb.resized, gb.crop, gb.flip), m
                assert (b.visual[m].blobs is not None) == b.kept
        kept_files = [p for c in part if c.kept for m in ("RGB", "Flow") for p in c.visual[m].paths]
        assert reads == kept_files
        assert len(headers) == 2 * (3 - len(keep))           # one header per visual modality of a foreign clip
    with pytest.raises(ValueError):
        ds.plan(idx, rng=np.random.RandomState(5), keep=[3])


def test_jpeg_frame_size_reads_the_header(tmp_path):
    from attention_based_tbn_amd.core.dataset.dataset import jpeg_frame_size
    from attention_based_tbn_amd.core.dataset.frames import jpeg_geometry
    from tests import jpeg_ref as R
    for name in R.color_names():
        path = tmp_path / "f.jpg"
        path.write_bytes(R.blob(name))
        geo = jpeg_geometry(R.blob(name))
        assert jpeg_frame_size(str(path)) == (geo.height, geo.width), name
    # a long application segment in front of the frame header: the reader goes past its first 64 KiB
    blob = R.blob(R.color_names()[0])
    geo = jpeg_geometry(blob)
    pad = b"\xff\xe1\xff\xff" + bytes(65533)
    (tmp_path / "g.jpg").write_bytes(blob[:2] + pad + pad + blob[2:])
    assert jpeg_frame_size(str(tmp_path / "g.jpg")) == (geo.height, geo.width)
    (tmp_path / "h.jpg").write_bytes(b"\xff\xd8\xff\xd9")
    with pytest.raises(Exception):
        jpeg_frame_size(str(tmp_path / "h.jpg"))


class _TwoTermModel(torch.nn.Module):
    """one weight; get_loss -> a mean-reduced class term and a prior term reduced as cfg says, with get_loss's multiplier"""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.w = torch.nn.Parameter(torch.tensor([0.5, -1.5]))

    def forward(self, x):
        return x * self.w

    def get_loss(self, criterion, target, out, epoch=0):
        att = self.cfg.model.attention
        mult = 0 if (self.training and epoch + 1 < att.decay_step) else att.wt_decay
        ce = (out[:, 0] ** 2).mean()
        rows = (out[:, 1] - target) ** 2
        prior = rows.sum() if att.loss_reduction == "sum" else rows.mean()
        return {"all_class": ce, "prior": prior, "total": ce + mult * prior}, out.shape[0]


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("k", [1, 2])
def test_train_step_scales_each_term_by_its_reduction(reduction, k):
    """the average over the ranks of what each rank back-propagates is the gradient of the loss on the global batch"""
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils import TrainStep
    cfg = load_config(["model.attention.enable=True", "model.attention.use_prior=True",
                       "model.attention.loss_reduction=" + reduction])
    epoch = cfg.model.attention.decay_step + 1
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0], [-2.0, 0.5]], dtype=torch.float64)
    t = torch.tensor([0.3, -0.2, 0.9], dtype=torch.float64)

    def grad_of(rows, share):
        model = _TwoTermModel(cfg).double()
        step = TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), None, accumulator_step=k)
        loss, _ = step(0, x[rows], t[rows], epoch, share=share)
        return model.w.grad.clone(), step.last_scale, loss

    whole, scale, _ = grad_of([0, 1, 2], None)
    assert scale is None
    g0, s0, l0 = grad_of([0], (1, 3, 2))
    g1, s1, l1 = grad_of([1, 2], (2, 3, 2))
    assert s0 == (2 / 3, 2 if reduction == "sum" else None) and s1 == (4 / 3, 2 if reduction == "sum" else None)
    assert torch.allclose((g0 + g1) / 2, whole, rtol=1e-12, atol=0)
    # the returned dictionary is the rank's own, un-scaled (divided by k as always)
    model = _TwoTermModel(cfg).double()
    want, _ = model.get_loss(None, t[[0]], model(x[[0]]), epoch)
    assert float(l0["total"].detach()) == pytest.approx(float(want["total"].detach()) / k, rel=1e-15)
    # equal shares: the mean factor is exactly one and is skipped -- loss["total"] itself is back-propagated
    ga, sa, la = grad_of([0, 1], (2, 4, 2))
    gb, sb, _ = grad_of([0, 1], None)
    assert sa == (None, 2 if reduction == "sum" else None)
    if reduction == "mean":
        assert torch.equal(ga, gb)
        model = _TwoTermModel(cfg).double()
        step = TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), None)
        loss = {"total": torch.ones((), requires_grad=True)}
        assert step._shared_total(loss, (2, 4, 2), epoch) is loss["total"]
        assert step._shared_total(loss, (3, 3, 1), epoch) is loss["total"]
    with pytest.raises(ValueError):
        grad_of([0], (0, 3, 2))
