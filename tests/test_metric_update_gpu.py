"""`tbn_metric_update` at operator level and `DeviceMetric` against `Metric`: a batch's hit counts (per head and all heads),
confusion matrices and loss terms in ONE launch, against `get_correct_score` (`tbn_topk_correct`) plus the arithmetic of
`Metric.set_metrics`.  Counts and integer-valued float atomics: every comparison is exact."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# heads (class counts) of one call; more than one head: slices of one wider matrix, side by side, so scores_ld > classes
HEAD_SETS = [[2], [63], [64], [65], [125], [352], [125, 352], [65, 2, 352, 64]]
BATCHES = [1, 3, 4, 5, 67]


def _topk_sets(min_classes):
    if min_classes <= 5:
        return [[1], [1, 2], [2, 1]]
    return [[1], [1, 5], [5, 1], [min_classes]]


def _update(scores, targets, topk, conf=None, losses=(), hits=None, loss_row=None, batch=None):
    """one `tbn_metric_update` call -> (hits (H + 1, nk) int32, loss_row); scores: 2-D views with stride(1) == 1"""
    from attention_based_tbn_amd._lib import MetricHead, call, ptr, stream_ptr
    H, nk = len(scores), len(topk)
    heads = (MetricHead * H)()
    for h in range(H):
        assert scores[h].stride(1) == 1 and scores[h].dtype == torch.float32 and targets[h].dtype == torch.int64
        heads[h] = MetricHead(ptr(scores[h]), scores[h].stride(0), scores[h].shape[1], ptr(targets[h]),
                              ptr(conf[h]) if conf is not None else 0)
    if hits is None:
        hits = torch.zeros((H + 1, nk), dtype=torch.int32, device="cuda")
    if loss_row is None:
        loss_row = torch.full((max(1, len(losses)),), -7.0, device="cuda")
    ptrs = (ctypes.c_void_p * max(1, len(losses)))(*[ptr(v) for v in losses])
    call("tbn_metric_update", heads, H, scores[0].shape[0] if batch is None else batch, (ctypes.c_int * nk)(*topk), nk,
         ptrs, len(losses), ptr(hits), ptr(loss_row), stream_ptr())
    return hits, loss_row


def _reference(scores, targets, topk):
    """(hits (H + 1, nk), [conf per head]) from `get_correct_score` and the sums / product rule of `Metric.set_metrics`"""
    from attention_based_tbn_amd.core.utils.metric import get_correct_score
    correct, confs = [], []
    for s, t in zip(scores, targets):
        corr, cm = get_correct_score(s.contiguous(), t, topk)
        correct.append(corr)
        confs.append(cm)
    rows = [[int(c[:k].sum()) for k in topk] for c in correct]
    joint = []
    for k in topk:
        c = correct[0][:k].sum(0)
        for c2 in correct[1:]:
            c = c * c2[:k].sum(0)
        joint.append(int(c.sum()))
    return torch.tensor(rows + [joint], dtype=torch.int32), confs


def _heads(classes, B, seed, pad=3):
    """random scores: one head contiguous (ld == classes); several: column slices of one matrix wider than their sum"""
    g = torch.Generator().manual_seed(seed)
    if len(classes) == 1:
        scores = [torch.randn(B, classes[0], generator=g).cuda()]
    else:
        wide = torch.randn(B, sum(classes) + pad, generator=g).cuda()
        scores, at = [], 0
        for c in classes:
            scores.append(wide[:, at:at + c])
            at += c
        assert scores[0].stride(0) > classes[0]
    targets = [torch.randint(0, c, (B,), generator=g).cuda() for c in classes]
    return scores, targets


@pytest.mark.parametrize("classes", HEAD_SETS, ids=lambda c: "x".join(map(str, c)))
def test_hits_confusion_and_losses_equal_topk_correct_and_the_metric_sums(classes):
    for B in BATCHES:
        scores, targets = _heads(classes, B, seed=1000 * B + sum(classes))
        if len(classes) > 1 and B > 2:     # make the all-heads row interesting: some samples hit everywhere at k = 1
            for s, t in zip(scores, targets):
                s[:B // 2].scatter_(1, t[:B // 2, None], 9.0)
        for topk in _topk_sets(min(classes)):
            want, want_conf = _reference(scores, targets, topk)
            conf = [torch.zeros(c, c, device="cuda") for c in classes]
            losses = [v for v in torch.randn(3, generator=torch.Generator().manual_seed(B)).cuda()]
            hits, loss_row = _update(scores, targets, topk, conf, losses)
            assert torch.equal(hits.cpu(), want), (B, topk, hits.cpu(), want)
            for h in range(len(classes)):
                assert torch.equal(conf[h], want_conf[h]), (B, topk, h)
                assert float(conf[h].sum()) == B
            assert torch.equal(loss_row.view(torch.int32), torch.stack(losses).view(torch.int32))
            # a second call ADDS into hits_row and the confusion matrices, and rewrites the losses
            _update(scores, targets, topk, conf, losses[:1], hits=hits, loss_row=loss_row)
            assert torch.equal(hits.cpu(), 2 * want) and torch.equal(conf[0], 2 * want_conf[0])
            assert torch.equal(loss_row[1:].view(torch.int32), torch.stack(losses[1:]).view(torch.int32))
        if len(classes) > 1 and B > 2:
            assert int(want[-1, 0]) >= B // 2


def test_wider_pitch_of_a_single_head_and_no_confusion_matrix():
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(9, 200, generator=g).cuda()
    scores = [wide[:, 17:17 + 125]]
    targets = [torch.randint(0, 125, (9,), generator=g).cuda()]
    want, _ = _reference(scores, targets, [1, 5])
    hits, loss_row = _update(scores, targets, [1, 5])
    assert torch.equal(hits.cpu(), want) and torch.equal(hits[0], hits[1])         # one head: the joint row is the head's
    assert float(loss_row[0]) == -7.0                                               # no losses: nothing written


def test_planted_rows_ties_missing_labels_and_nans():
    C, topk = 65, [1, 2, 5]
    g = torch.Generator().manual_seed(11)
    s = torch.randn(7, C, generator=g)
    t = torch.randint(0, C, (7,), generator=g)
    s[0] = 0.25                          # all equal: ranks are the class indices
    t[0] = 3                             # -> position 3: a hit at k = 5 only
    s[1, 10] = s[1, 40] = 50.0           # duplicated maximum, the target the higher index of the pair
    t[1] = 40                            # -> a miss at k = 1, a hit at k = 2
    t[2] = -1                            # no label: no hit, no confusion entry
    s[3, int(t[3])] = float("nan")       # NaN at the target: no hit
    t[4] = 20
    s[4, 20] = 60.0
    s[4, 5] = float("nan")               # NaN elsewhere: never ranked, the target stays first
    s[5, 64] = float("inf")              # the last lane-strided element wins
    t[5] = 64
    s[6] = float("-inf")                 # all -inf: an all-equal row
    t[6] = 0
    scores, targets = [s.cuda()], [t.cuda()]
    conf = [torch.zeros(C, C, device="cuda")]
    hits, _ = _update(scores, targets, topk, conf)
    want, want_conf = _reference(scores, targets, topk)
    assert torch.equal(hits.cpu(), want) and torch.equal(conf[0], want_conf[0])
    # and what those rows must give, spelled out: hits at k=1: rows 4, 5, 6; k=2: + row 1; k=5: + row 0
    assert hits[0].tolist() == [3, 4, 5] and hits[1].tolist() == [3, 4, 5]
    assert float(conf[0].sum()) == 6 and float(conf[0][40, 10]) == 1 and float(conf[0][3, 0]) == 1
    # second head whose rows all hit: the joint row then equals the first head's, and a -1 there zeroes its sample
    s2 = torch.zeros(7, 4)
    t2 = torch.tensor([1, 1, 1, 1, 1, 1, -1])
    s2[:, 1] = 1.0
    both = [scores[0], s2.cuda()], [targets[0], t2.cuda()]
    hits, _ = _update(both[0], both[1], [1, 2])
    want, _ = _reference(both[0], both[1], [1, 2])
    assert torch.equal(hits.cpu(), want) and hits.tolist() == [[3, 4], [6, 6], [2, 3]]


def test_empty_batch_still_copies_the_losses():
    scores, targets = _heads([5], 1, seed=0)
    losses = [torch.tensor(1.5, device="cuda"), torch.tensor(-0.0, device="cuda")]
    hits, loss_row = _update(scores, targets, [1], losses=losses, batch=0)
    assert hits.tolist() == [[0], [0]]
    assert torch.equal(loss_row.view(torch.int32), torch.stack(losses).view(torch.int32))
    hits, _ = _update(scores, targets, [1], batch=0)
    assert hits.tolist() == [[0], [0]]


def test_refusals():
    from attention_based_tbn_amd._lib import MetricHead, TbnHipError, call, ptr
    scores, targets = _heads([5, 9], 3, seed=0)
    hits = torch.zeros(3, 2, dtype=torch.int32, device="cuda")
    row = torch.zeros(8, device="cuda")
    one = torch.zeros((), device="cuda")

    def attempt(heads=None, H=2, batch=3, topk=(1, 2), nk=None, losses=(one,), nl=None, hits_p=None, row_p=None,
                null_heads=False, null_topk=False, null_loss=False):
        if heads is None:
            heads = [(ptr(s), s.stride(0), s.shape[1], ptr(t), 0) for s, t in zip(scores, targets)]
        arr = (MetricHead * 5)(*[MetricHead(*h) for h in heads])
        ks = (ctypes.c_int * 9)(*topk)
        ptrs = (ctypes.c_void_p * 9)(*[ptr(v) if v is not None else None for v in losses])
        with pytest.raises(TbnHipError, match="metric_update:"):
            call("tbn_metric_update", None if null_heads else arr, H, batch, None if null_topk else ks,
                 len(topk) if nk is None else nk, None if null_loss else ptrs, len(losses) if nl is None else nl,
                 ptr(hits) if hits_p is None else hits_p, ptr(row) if row_p is None else row_p, None)

    attempt(null_heads=True)
    attempt(null_topk=True)
    attempt(null_loss=True)
    attempt(hits_p=0)
    attempt(row_p=0)
    attempt(losses=(one, None))
    s, t = scores[0], targets[0]
    attempt(heads=[(0, 5, 5, ptr(t), 0), (ptr(s), s.stride(0), 5, ptr(t), 0)])
    attempt(heads=[(ptr(s), s.stride(0), 5, 0, 0), (ptr(s), s.stride(0), 5, ptr(t), 0)])
    attempt(H=0)
    attempt(H=5)
    attempt(nk=0)
    attempt(topk=(1,) * 9)
    attempt(topk=(0, 1))
    attempt(topk=(1, 6))                     # 6 > the 5 classes of head 0, though head 1 has 9
    attempt(nl=-1)
    attempt(losses=(one,) * 9)
    attempt(batch=-1)
    attempt(heads=[(ptr(s), 4, 5, ptr(t), 0), (ptr(s), s.stride(0), 5, ptr(t), 0)])       # scores_ld < classes
    assert int(hits.sum()) == 0


# ---------------------------------------------------------------------------------------------- DeviceMetric vs Metric
SIZES = (4, 4, 4, 4, 3)


def _cfg(attention):
    from attention_based_tbn_amd.config import load_config
    on = ["model.attention.enable=True", "model.attention.use_fixed=False", "model.attention.use_prior=True",
          "model.attention.use_contrast=True", "model.attention.use_entropy=True"]
    return load_config(["val.topk=[1,5]"] + (on if attention else ["model.attention.enable=False"]))


def _stream_of_batches(cfg, sizes, keys, seed=0):
    """[(out, target, B, loss)]: two heads side by side in one matrix (as `Classifier.shared_scores` lays them), device
    scalar losses"""
    g = torch.Generator().manual_seed(seed)
    n_verb, n_noun = cfg.model.num_classes["verb"], cfg.model.num_classes["noun"]
    items = []
    for B in sizes:
        wide = torch.randn(B, n_verb + n_noun, generator=g).cuda()
        tv, tn = torch.randint(0, n_verb, (B,), generator=g).cuda(), torch.randint(0, n_noun, (B,), generator=g).cuda()
        wide[:B // 2].scatter_(1, tv[:B // 2, None], 9.0)
        wide[:B // 2 + 1, n_verb:].scatter_(1, tn[:B // 2 + 1, None], 9.0)
        out = {"verb": wide[:, :n_verb], "noun": wide[:, n_verb:], "weights": torch.rand(B, 3, generator=g).cuda()}
        vals = (torch.rand(len(keys), generator=g) * 3).cuda()
        items.append((out, {"class": {"verb": tv, "noun": tn}}, B, {k: vals[i] for i, k in enumerate(keys)}))
    return items


def _feed(metric, items):
    for out, target, B, loss in items:
        metric.set_metrics(out, target, B, loss)
    return metric.get_metrics()


@pytest.mark.parametrize("attention", [False, True])
def test_device_metric_equals_metric(attention):
    from attention_based_tbn_amd.core.utils import DeviceMetric, Metric
    cfg = _cfg(attention)
    dev = torch.device("cuda")
    ref, got = Metric(cfg, len(SIZES), dev), DeviceMetric(cfg, len(SIZES), dev)
    keys = list(ref.loss.keys())
    assert keys == list(got.loss.keys()) and ("prior" in keys) == attention and "all_class" in keys
    items = _stream_of_batches(cfg, SIZES, keys)
    want, have = _feed(ref, items), _feed(got, items)
    assert have[0] == want[0] and have[1] == want[1], (have[:2], want[:2])
    assert list(have[0].keys()) == list(want[0].keys()) and list(have[1].keys()) == list(want[1].keys())
    assert all(isinstance(v, float) for v in have[0].values())
    assert 0 < have[1]["all_class"][0] <= have[1]["verb"][0] < 100          # neither nothing nor everything is right
    for k in ("verb", "noun"):
        assert torch.equal(have[2][k], want[2][k]) and float(have[2][k].sum()) == sum(SIZES)


def test_running_loss_and_host_numbers():
    from attention_based_tbn_amd.core.utils import DeviceMetric
    cfg = _cfg(False)
    metric = DeviceMetric(cfg, 5, torch.device("cuda"))
    keys = list(metric.loss.keys())
    items = _stream_of_batches(cfg, SIZES, keys, seed=2)
    total = 0.0
    for i, (out, target, B, loss) in enumerate(items):
        loss = dict(loss)
        if i % 2:
            loss["verb"] = 0.5 * i                       # a Python number stays on the host
        metric.set_metrics(out, target, B, loss)
        total += float(loss["total"])
        assert metric.running("total") == total and metric.running() == total
    assert metric.get_metrics()[0]["total"] == round(total / 5, 5)
    want_verb = sum(float(items[i][3]["verb"]) if i % 2 == 0 else 0.5 * i for i in range(5))
    assert metric.loss["verb"] == round(want_verb / 5, 5)


def test_set_metrics_never_synchronises(monkeypatch):
    from attention_based_tbn_amd.core.utils import DeviceMetric, Metric
    cfg = _cfg(True)
    dev = torch.device("cuda")
    ref, got = Metric(cfg, len(SIZES), dev), DeviceMetric(cfg, len(SIZES), dev)
    items = _stream_of_batches(cfg, SIZES, list(ref.loss.keys()), seed=1)
    want = _feed(ref, items)

    def forbidden(*a, **kw):
        raise AssertionError("host synchronisation inside set_metrics")
    with monkeypatch.context() as m:
        for name in ("item", "tolist", "cpu", "numpy", "__float__"):
            m.setattr(torch.Tensor, name, forbidden)
        for out, target, B, loss in items:
            got.set_metrics(out, target, B, loss)
        with pytest.raises(AssertionError, match="host synchronisation"):           # the patch bites
            Metric(cfg, len(SIZES), dev).set_metrics(*items[0])
    have = got.get_metrics()
    assert have[0] == want[0] and have[1] == want[1]


def test_ring_flush_keeps_the_sums():
    from attention_based_tbn_amd.core.utils import DeviceMetric, Metric
    cfg = _cfg(False)
    dev = torch.device("cuda")
    ref, got = Metric(cfg, 2, dev), DeviceMetric(cfg, 2, dev)
    assert got._cap == 8
    items = _stream_of_batches(cfg, (4, 3, 4, 1, 2, 4, 4, 3, 5, 4, 4, 2), list(ref.loss.keys()), seed=3)
    want, have = _feed(ref, items), _feed(got, items)
    assert have[0] == want[0] and have[1] == want[1]
    for k in ("verb", "noun"):
        assert torch.equal(have[2][k], want[2][k])
