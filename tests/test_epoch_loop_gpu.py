"""The epoch loop on the device: batches prefetched on the loader's thread and side stream equal those of the synchronous
twin bit for bit, and the loops of `core.tools` (train / validate / test / run_trainer / run_tester) run on them."""
import logging
import os
import threading

import numpy as np
import pytest
import torch

from tests import clip_loader_util as U

pytestmark = pytest.mark.gpu

MODALITY = ["RGB", "Flow", "Audio"]
LOG = logging.getLogger("epoch_loop_test")


def _same(a, b, path="batch"):
    """nested equality of two batches: tensors bit for bit on the same device, containers by type and keys"""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.device == b.device and a.dtype == b.dtype, path
        assert a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert type(a) is type(b) and list(a.keys()) == list(b.keys()), path
        for k in a:
            _same(a[k], b[k], path + "." + str(k))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "{}[{}]".format(path, i))
    else:
        assert a == b, path


@pytest.mark.parametrize("mode,sampling,extra", [
    ("train", "async", ["model.attention.use_prior=True", "model.attention.prior_type=loud"]),
    ("train", "sync", ["model.attention.use_fixed=True"]),
    ("val", "sync", ["model.attention.enable=False"])])
def test_prefetched_batches_equal_the_synchronous_twin(tmp_path, mode, sampling, extra):
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils import ClipLoader
    cfg = load_config(U.write_dataset(tmp_path) + ["data.sampling=" + sampling] + extra)
    ds = U.make_dataset(cfg, MODALITY, mode)
    for batch_size in (1, 2):
        for prefetch in (1, 2):
            torch.manual_seed(17 + batch_size)
            np.random.seed(3)
            state = np.random.get_state()[1].copy()
            twin = list(ClipLoader(ds, batch_size, shuffle=(mode == "train"), prefetch=0, rng="private"))
            torch.manual_seed(17 + batch_size)
            loader = ClipLoader(ds, batch_size, shuffle=(mode == "train"), prefetch=prefetch)
            got = []
            for batch in loader:
                # used right away on the consumer's stream, while the producer is at work on the next one
                got.append((batch, batch[0]["RGB"].sum() + batch[0]["Audio"].sum()))
            assert len(got) == len(twin) == -(-3 // batch_size)
            for (batch, total), want in zip(got, twin):
                assert len(batch) == (2 if mode == "train" else 3)
                _same(batch, want)
                assert torch.equal(total, want[0]["RGB"].sum() + want[0]["Audio"].sum())
            assert np.array_equal(np.random.get_state()[1], state)          # the global NumPy generator is not drawn from
    if mode == "train":      # another torch seed: another epoch (the comparison above is not between constants)
        torch.manual_seed(99)
        other = list(ClipLoader(ds, 1, shuffle=True, prefetch=2))
        assert any(not torch.equal(a[0]["RGB"], b[0]["RGB"]) for a, b in zip(other, twin[:3])) or \
            [a[0]["vid_id"] for a in other] != [b[0]["vid_id"] for b in twin[:3]]


def test_private_twin_equals_the_global_path_seeded_alike(tmp_path):
    """a `RandomState(seed)` and the global generator after `np.random.seed(seed)` are one stream: the private pass is the
    parent's synchronous pass, drawn from elsewhere"""
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.utils import ClipLoader
    cfg = load_config(U.write_dataset(tmp_path) + ["data.sampling=async", "model.attention.enable=False"])
    ds = U.make_dataset(cfg, MODALITY, "train")
    torch.manual_seed(5)
    private = list(ClipLoader(ds, 2, shuffle=True, prefetch=2))
    torch.manual_seed(5)
    torch.randperm(3)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
    torch.manual_seed(5)
    np.random.seed(seed)
    for got, want in zip(private, ClipLoader(ds, 2, shuffle=True)):
        _same(got, want)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    from attention_based_tbn_amd.config import get_modality, load_config
    root = tmp_path_factory.mktemp("epoch_loop")
    cfg = load_config(U.write_big_dataset(root) + [
        "model.attention.enable=False", "model.fusion_dropout=0", "val.vid_list=", "test.vid_list=",
        "test.annotation_file=ann.csv", "val.num_segments=2", "test.num_segments=2", "val.batch_size=2",
        "test.batch_size=2", "train.epochs=1", "out_dir=" + str(root), "exp_name=loop"])
    return cfg, get_modality(cfg), str(root)


def test_train_validate_and_test_loops(big):
    from attention_based_tbn_amd.core import tools
    from attention_based_tbn_amd.core.models import build_model
    from attention_based_tbn_amd.core.utils import Metric, build_optimizer, create_dataloader
    cfg, modality, _ = big
    dev = torch.device("cuda")
    torch.manual_seed(0)
    np.random.seed(0)
    model, criterion, _ = build_model(cfg, modality, dev)
    optimizer, scheduler, _ = build_optimizer(cfg, model)
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    LOG.addHandler(handler)
    LOG.setLevel(logging.INFO)
    try:
        loader = create_dataloader(cfg, LOG, modality, "train", prefetch=2)
        before = model.Base_RGB.flat_weight.detach().clone()
        train_loss = tools.train(cfg, model, loader, optimizer, scheduler, criterion, 0, LOG, dev)
    finally:
        LOG.removeHandler(handler)
    assert set(train_loss) == {"verb", "noun", "all_class", "total"}
    assert all(isinstance(v, float) and np.isfinite(v) and v > 0 for v in train_loss.values())
    assert not torch.equal(before, model.Base_RGB.flat_weight)                  # the optimiser stepped
    lines = [r.getMessage() for r in records if "Batch Progress" in r.getMessage()]
    assert [ln.split(" ||")[0] for ln in lines] == ["Batch Progress: [1/2]", "Batch Progress: [2/2]"]
    assert not [t for t in threading.enumerate() if t.name == "ClipLoader-producer" and t.is_alive()]

    # validate on prefetched batches with DeviceMetric == the same loop with Metric on the synchronous loader
    val_loader = create_dataloader(cfg, LOG, modality, "val", prefetch=2)
    val_loss, val_acc, conf = tools.validate(cfg, model, val_loader, criterion, modality, LOG, dev)
    ref = Metric(cfg, 3 // 2, dev)
    with torch.no_grad():
        for data, target, _ in create_dataloader(cfg, LOG, modality, "val"):
            out = model(data)
            loss, B = model.get_loss(criterion, target, out)
            ref.set_metrics(out, target, B, loss)
    want_loss, want_acc, want_conf = ref.get_metrics()
    assert val_acc == want_acc
    # fp32 sums whose order may differ between two runs of the forward (relative 1e-6), rounded to 5 decimals
    assert val_loss.keys() == want_loss.keys()
    for k in val_loss:
        assert val_loss[k] == pytest.approx(want_loss[k], rel=1e-4, abs=2e-5), k
    for k in conf:
        assert torch.equal(conf[k], want_conf[k]) and float(conf[k].sum()) == 3

    # test(): three elements, four with save_results
    test_loader = create_dataloader(cfg, LOG, modality, "test", prefetch=2)
    res = tools.test(cfg, model, test_loader, criterion, modality, LOG, dev)
    assert len(res) == 3 and res[1].keys() == val_acc.keys() and torch.equal(res[2]["verb"], conf["verb"])
    cfg.test.save_results = True
    try:
        res = tools.test(cfg, model, test_loader, criterion, modality, LOG, dev)
    finally:
        cfg.test.save_results = False
    assert len(res) == 4 and list(res[3].keys()) == ["action_id", "verb", "noun"]
    assert torch.cat(res[3]["action_id"]).tolist() == [11, 12, 13]
    assert [tuple(t.shape) for t in res[3]["verb"]] == [(2, 125), (1, 125)]


class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, epoch):
        self.rows.append((tag, float(value), epoch))


@pytest.fixture(scope="module")
def trained(big):
    """one epoch of `run_trainer` on prefetched batches -> (checkpoint path, the writer's rows)"""
    from attention_based_tbn_amd.core import tools
    cfg, modality, root = big
    writer = _Writer()
    torch.manual_seed(1)
    np.random.seed(1)
    tools.run_trainer(cfg, LOG, modality, writer)
    assert cfg.data.dataset == "epic" and cfg.model.arch == "bninception"
    path = os.path.join(root, cfg.model.checkpoint_dir, "loop", "epic_tbn_bninception_" + "_".join(modality) + ".pth")
    return path, writer.rows


def test_run_trainer_writes_the_checkpoint_and_the_scalars(trained):
    path, rows = trained
    assert os.path.exists(path)
    data = torch.load(path, map_location="cpu", weights_only=False)
    assert data["epoch"] == 0 and len(data["train_loss"]) == 1 and len(data["validation_loss"]) == 1
    assert set(data["validation_accuracy"].keys()) == {"verb", "noun"} and "scheduler" in data and "conf_mat" in data
    tags = [r[0] for r in rows]
    assert tags[0] == "train/learning_rate" and all(r[2] == 0 for r in rows)
    for tag in ("train/total_loss", "val/total_loss", "train/verb_loss", "val/accuracy/verb_top_1",
                "val/accuracy/all_class_top_5"):
        assert tag in tags, tag
    assert not [t for t in threading.enumerate() if t.name == "ClipLoader-producer" and t.is_alive()]


def test_run_trainer_resumes(big, trained):
    """epochs += start_epoch (reference train.py:229-233): one more epoch, the histories grow; without validation"""
    from attention_based_tbn_amd.core import tools
    cfg, modality, _ = big
    path, _ = trained
    cfg.train.pre_trained, cfg.val.enable = path, False
    try:
        tools.run_trainer(cfg, LOG, modality, prefetch=0)
    finally:
        cfg.train.pre_trained, cfg.val.enable = "", True
    data = torch.load(path, map_location="cpu", weights_only=False)
    assert data["epoch"] == 1 and len(data["train_loss"]) == 2 and len(data["validation_loss"]) == 1
    assert "conf_mat" not in data


def test_run_tester_reads_the_checkpoint(big, trained):
    """one loader per annotation file; the missing action-name table is logged, not raised, as in the reference"""
    from attention_based_tbn_amd.core import tools
    cfg, modality, root = big
    records = []
    handler = logging.Handler()
    handler.emit = records.append
    LOG.addHandler(handler)
    LOG.setLevel(logging.INFO)
    cfg.test.pre_trained, cfg.test.save_results = trained[0], True
    cfg.test.annotation_file, cfg.test.results_file = ["ann.csv"], ["seen.json"]
    try:
        tools.run_tester(cfg, LOG, modality)
    finally:
        LOG.removeHandler(handler)
        cfg.test.pre_trained, cfg.test.save_results, cfg.test.annotation_file = "", False, "ann.csv"
    text = [r.getMessage() for r in records]
    assert "3 action segments to be processed." in text and any(t.startswith("Test_Loss: {") for t in text)
    assert any(r.levelno == logging.ERROR for r in records)
    assert not os.path.exists(os.path.join(root, "inferences", "seen.json"))
