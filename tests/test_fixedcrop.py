"""Multi-crop test pipeline (reference core/dataset/transform.py:106-179 `FixedCrop`, then `Stack` :415-461) and the
rest of the transform import surface of the reference's tools.

Expected values: tests/golden/fixedcrop.npz, written by the unmodified reference classes (cv2.resize stubbed by the
restated INTER_LINEAR, parity unpinned as before -- tests/golden/make_golden_fixedcrop.py), and NumPy slicing written
here (`np_fixed_crop`), which the CPU tests first check against that fixture.
CPU: import lines, window tables, refusals, TransferTensorDict, the C-ABI export / capability bit / host validation.
GPU: `tbn_frames_to_tensor_crops` through DevicePipeline and through the reference-style chain, bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import transform as otf

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PKG = "attention_based_tbn_amd.core.dataset.transform"


def _fixture():
    meta = json.load(open(os.path.join(GOLD, "fixedcrop.json")))
    return meta["cases"], np.load(os.path.join(GOLD, "fixedcrop.npz"))


def _size(case):
    return case["size"] if isinstance(case["size"], int) else tuple(case["size"])


def closed_form_windows(img_h, img_w, size, locations):
    """(x1, y1) per location: 0 centre (floor division), 1 top left, 2 top right, 3 bottom left, 4 bottom right"""
    h, w = (size, size) if isinstance(size, int) else size
    table = [((img_w - w) // 2, (img_h - h) // 2), (0, 0), (img_w - w, 0), (0, img_h - h), (img_w - w, img_h - h)]
    return [table[loc] for loc in locations]


def np_fixed_crop(imgs, size, locations, horizontal_flip):
    """the flat list in the reference's order: windows outermost, then the images, then plain / mirrored"""
    h, w = (size, size) if isinstance(size, int) else size
    out = []
    for x1, y1 in closed_form_windows(imgs[0].shape[0], imgs[0].shape[1], size, locations):
        for im in imgs:
            out.append(im[y1:y1 + h, x1:x1 + w])
            if horizontal_flip:
                out.append(np.fliplr(out[-1]))
    return out


def np_case(case, frames):
    imgs = list(frames)
    if case["rescale"]:
        imgs = otf.rescale(imgs, case["rescale"])
    imgs = np_fixed_crop(imgs, _size(case), case["locations"], case["horizontal_flip"])
    return otf.stack_totensor_normalize(imgs, case["modality"], case["mean"], case["std"])


def fused(case, device="cuda"):
    from attention_based_tbn_amd.core.dataset import DevicePipeline, FixedCrop, Rescale
    geo = ([Rescale(case["rescale"])] if case["rescale"] else []) + [
        FixedCrop(_size(case), locations=case["locations"], horizontal_flip=case["horizontal_flip"])]
    return DevicePipeline(case["modality"], geo, case["mean"], case["std"], device=device)


def chain(case):
    """the reference's composition, core/tools/test.py:136-171"""
    from attention_based_tbn_amd.core.dataset import FixedCrop, Normalize, Rescale, Stack, ToTensor
    return ([Rescale(case["rescale"])] if case["rescale"] else []) + [
        FixedCrop(_size(case), locations=case["locations"], horizontal_flip=case["horizontal_flip"]),
        Stack(case["modality"]), ToTensor(), Normalize(case["mean"], case["std"])]


def compose(ts, x):
    for t in ts:
        x = t(x)
    return x


# ----------------------------------------------------------------------------------------------- CPU
def test_reference_tool_import_lines_work_against_the_product_package():
    """reference core/tools/train.py:21 and core/tools/test.py:16-24 with the package name swapped"""
    ns = {}
    exec(f"from {PKG} import TransferTensorDict", ns)
    exec(f"from {PKG} import (\n    Rescale,\n    FixedCrop,\n    CenterCrop,\n    Stack,\n    ToTensor,\n"
         "    Normalize,\n    TransferTensorDict,\n)", ns)
    import attention_based_tbn_amd.core.dataset as ds
    for name in ("Rescale", "FixedCrop", "CenterCrop", "Stack", "ToTensor", "Normalize", "TransferTensorDict",
                 "RandomCrop", "RandomHorizontalFlip", "MultiScaleCrop", "DevicePipeline", "get_transforms"):
        assert callable(getattr(ds, name)), name
    # the reference's constructor arguments
    ns["FixedCrop"](224, locations=[0, 1, 2, 3, 4], horizontal_flip=True)
    ns["Stack"]("Flow", length=10)
    ns["ToTensor"](is_audio=True)
    ns["Normalize"]([0.5], [1.0])
    ns["TransferTensorDict"](torch.device("cpu"))


def test_numpy_restatement_of_fixedcrop_matches_reference_fixture():
    """the slicing the GPU tests compare against, checked first against what the reference classes wrote"""
    cases, z = _fixture()
    assert [c["name"][0] for c in cases] == list("abcdef")
    for k, case in enumerate(cases):
        got = np_case(case, z["in%d" % k])
        assert list(got.shape) == case["shape"], case["name"]
        assert np.array_equal(got, z["out%d" % k]), case["name"]
    # (d): 100 list entries -> a Flow stack alternates plain and mirrored images of five frames
    d, frames = cases[3], z["in3"]
    assert d["shape"][0] == 10 and d["horizontal_flip"] and d["modality"] == "Flow"
    x1, y1 = closed_form_windows(41, 57, 24, [0])[0]
    raw = (z["out3"][0] * np.float32(d["std"][0]) + np.float32(d["mean"][0])) * 255
    for u in range(10):
        want = frames[u // 2][y1:y1 + 24, x1:x1 + 24]
        assert np.abs(raw[u] - (np.fliplr(want) if u % 2 else want)).max() < 1e-2, u


def test_fixedcrop_window_tables_equal_the_closed_form():
    from attention_based_tbn_amd.core.dataset import FixedCrop, Rescale
    from attention_based_tbn_amd.core.dataset.transform import _Geometry
    cases, z = _fixture()
    for k, case in enumerate(cases):
        h, w = case["hw"]
        geo = _Geometry(h, w)
        if case["rescale"]:
            Rescale(case["rescale"])(geo)
            h, w = otf.rescale([z["in%d" % k][0]], case["rescale"])[0].shape[:2]
        fc = FixedCrop(_size(case), locations=case["locations"], horizontal_flip=case["horizontal_flip"])
        want = closed_form_windows(h, w, _size(case), case["locations"])
        assert fc.windows(h, w) == want, case["name"]
        assert fc(geo) is geo
        assert geo.windows == want and geo.mirror == (2 if case["horizontal_flip"] else 0), case["name"]
        ch, cw = (_size(case),) * 2 if isinstance(_size(case), int) else _size(case)
        assert (geo.h, geo.w) == (ch, cw)
    # both margins of 41x57 - 24 are odd: the centre floors
    assert closed_form_windows(41, 57, 24, [0]) == [(16, 8)]
    # a flip recorded before mirrors every window: window x of the mirrored frame, seen from the source
    from attention_based_tbn_amd.core.dataset import RandomHorizontalFlip
    for pairs, mode in ((False, 1), (True, 3)):
        geo = _Geometry(41, 57)
        RandomHorizontalFlip(prob=1.0)(geo)
        FixedCrop(24, [0, 1, 4], horizontal_flip=pairs)(geo)
        assert geo.windows == [(57 - 16 - 24, 8), (33, 0), (0, 17)] and geo.mirror == mode


def test_fixedcrop_and_get_transforms_refusals():
    from attention_based_tbn_amd._lib import TbnHipError
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import (CenterCrop, FixedCrop, MultiScaleCrop, RandomCrop,
                                                      RandomHorizontalFlip, Rescale, get_transforms)
    from attention_based_tbn_amd.core.dataset.transform import _Geometry
    for later in (CenterCrop(8), Rescale(16), RandomHorizontalFlip(prob=1.0), RandomHorizontalFlip(prob=0.0),
                  MultiScaleCrop(8), RandomCrop(8), FixedCrop(8)):
        geo = _Geometry(41, 57)
        FixedCrop(24)(geo)
        with pytest.raises(TbnHipError, match="after FixedCrop"):
            later(geo)
    for bad in ([5], [0, -1], [0, "centre"]):
        with pytest.raises(TbnHipError, match="unknown location"):
            FixedCrop(24, locations=bad)
    with pytest.raises(TbnHipError, match="locations"):
        FixedCrop(24, locations=[0] * 17)
    with pytest.raises(TbnHipError, match="outside"):
        FixedCrop(64)(_Geometry(41, 57))
    cfg = load_config([])
    for bad in (0, 2, 3, 20, None):
        with pytest.raises(TbnHipError, match="test_crops"):
            get_transforms(cfg, ["RGB", "Flow"], "test", test_crops=bad)
    # train ignores it; the defaults are today's
    tf = get_transforms(cfg, ["RGB", "Flow"], "train", test_crops=7)
    assert [type(t).__name__ for t in tf["RGB"].geometry] == ["MultiScaleCrop", "RandomHorizontalFlip"]
    assert [type(t).__name__ for t in get_transforms(cfg, ["RGB"], "test")["RGB"].geometry] == ["Rescale", "CenterCrop"]
    for k, flip in ((5, False), (10, True)):
        fc = get_transforms(cfg, ["RGB", "Flow", "Audio"], "test", test_crops=k)["Flow"].geometry[-1]
        assert isinstance(fc, FixedCrop) and fc.locations == [0, 1, 2, 3, 4] and fc.horizontal_flip is flip
        assert fc.size == (cfg.data.test_crop_size,) * 2


def test_geometry_classes_take_frames_and_return_a_recorded_sample():
    """the reference's argument (a list of frames) starts a recorded sample; Stack adds modality and length"""
    from attention_based_tbn_amd.core.dataset import CenterCrop, Rescale, Stack
    frames = [np.zeros((41, 57, 3), np.uint8)] * 2
    s = Rescale(32)(frames)
    assert s.frames is frames and s.geo.resized == (44, 32)
    assert CenterCrop(24)(s) is s and s.geo.crop == [10, 4, 24, 24]
    assert Stack("RGB")(s) is s and (s.modality, s.length) == ("RGB", 1)
    f = Stack("Flow", length=5)([np.zeros((41, 57), np.uint8)] * 10)
    assert (f.modality, f.length) == ("Flow", 5) and f.geo.box == [0, 0, 57, 41]


def test_transfer_tensor_dict_keeps_dtypes_and_other_values():
    from attention_based_tbn_amd.core.dataset import TransferTensorDict
    frames = torch.arange(24, dtype=torch.uint8).reshape(1, 2, 4, 3)
    d = {"RGB": frames, "indices": {"RGB": [1, 2, 3], "t": torch.tensor([4, 5])},
         "target": {"class": {"verb": torch.tensor([3]), "noun": torch.tensor([7])}, "weights": torch.ones(2, 3)},
         "name": "P01_01", "n": 3, "none": None}
    out = TransferTensorDict(torch.device("cpu"))(d)
    assert out["RGB"].dtype == torch.uint8 and torch.equal(out["RGB"], frames)
    assert out["indices"]["RGB"] == [1, 2, 3] and out["indices"]["t"].dtype == torch.int64
    assert out["target"]["class"]["noun"].item() == 7 and out["target"]["weights"].dtype == torch.float32
    assert out["name"] == "P01_01" and out["n"] == 3 and out["none"] is None
    with pytest.raises(AssertionError):
        TransferTensorDict("cpu")


def test_library_exports_the_crops_entry_and_validates_on_the_host():
    """as tests/test_host_cpu.py does for the single-window entry: a negative code and a message naming the entry,
    with pointers that are never dereferenced"""
    from attention_based_tbn_amd._lib import SIGNATURES, lib
    L = lib()
    assert "tbn_frames_to_tensor_crops" in SIGNATURES and callable(L.tbn_frames_to_tensor_crops)
    assert L.tbn_capabilities() & 4
    assert L.tbn_version() & 0xFFFF == 102
    bad = 0x1000

    def fails(needle, n_img=4, hw=(64, 64), c=3, box=(0, 0, 64, 64), resized=(64, 64), xs=(0,), ys=(0,), n_crops=None,
              out=(32, 32), mirror=0, stack=1):
        k = len(xs) if n_crops is None else n_crops
        ax, ay = (C.c_int * max(1, len(xs)))(*xs), (C.c_int * max(1, len(ys)))(*ys)
        rc = L.tbn_frames_to_tensor_crops(bad, n_img, hw[0], hw[1], c, *box, *resized, ax, ay, k, out[0], out[1],
                                          mirror, stack, None, None, 0, 1, bad, None)
        assert rc < 0, rc
        msg = L.tbn_last_error().decode()
        assert "frames_to_tensor_crops" in msg and needle in msg, msg

    fails("bad frame stack", n_img=3, c=1, xs=(0, 8, 16), ys=(0, 0, 0), stack=10)      # 9 entries, stack 10
    fails("bad frame stack", n_img=5, c=1, xs=(0,) * 5, ys=(0,) * 5, mirror=1, stack=10)  # 25: a mirror-1 list has no pairs
    fails("outside the resized", xs=(0, 33), ys=(0, 0))
    fails("outside the resized", xs=(0, 0), ys=(0, -1))
    fails("outside the resized", resized=(40, 40), xs=(8, 9), ys=(8, 8))
    fails("crop windows", n_crops=0)
    fails("crop windows", xs=(0,) * 17, ys=(0,) * 17)
    fails("mirror mode", mirror=4)
    fails("outside the 64x64 frame", box=(10, 10, 60, 60))
    rc = L.tbn_frames_to_tensor_crops(bad, 4, 64, 64, 3, 0, 0, 64, 64, 64, 64, None, None, 1, 32, 32, 0, 1, None, None,
                                      0, 1, bad, None)
    assert rc < 0 and "null argument" in L.tbn_last_error().decode()


# ----------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(6))
def test_fixture_parity_fused_and_reference_style_chain(k):
    cases, z = _fixture()
    case, frames = cases[k], [f for f in z["in%d" % k]]
    want = z["out%d" % k]
    got = fused(case)(frames)
    assert got.is_cuda and got.dtype == torch.float32 and list(got.shape) == case["shape"]
    assert np.array_equal(got.cpu().numpy(), want), ("DevicePipeline", case["name"])
    got = compose(chain(case), frames)
    assert got.is_cuda and list(got.shape) == case["shape"]
    assert np.array_equal(got.cpu().numpy(), want), ("chain", case["name"])
    # a uint8 tensor already on the device is accepted by both
    t = torch.from_numpy(np.stack(frames, 0).reshape(len(frames), 41, 57, -1)).cuda()
    assert np.array_equal(fused(case)(t).cpu().numpy(), want)
    assert np.array_equal(compose(chain(case), t).cpu().numpy(), want)


def _raw_crops(frames, box, resized, xs, ys, out_wh, mirror, stack, stat=None, guard=4096):
    """tbn_frames_to_tensor_crops straight through ctypes into a buffer with NaN guard regions on both sides"""
    from attention_based_tbn_amd._lib import call, ptr, stream_ptr
    n, H, W, c = frames.shape
    rows = n * len(xs) * (2 if mirror >= 2 else 1) // stack
    numel = rows * c * stack * out_wh[0] * out_wh[1]
    buf = torch.full((guard + numel + guard,), float("nan"), device="cuda")
    ax, ay = (C.c_int * len(xs))(*xs), (C.c_int * len(ys))(*ys)
    mean, std = stat if stat else (None, None)
    call("tbn_frames_to_tensor_crops", ptr(frames), n, H, W, c, *box, *resized, ax, ay, len(xs), out_wh[0], out_wh[1],
         mirror, stack, ptr(mean), ptr(std), 0 if mean is None else mean.numel(), 1, buf.data_ptr() + 4 * guard,
         stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + numel:]).all()), "guard written"
    body = buf[guard:guard + numel]
    assert not bool(torch.isnan(body).any()), "an output element was not written"
    return body.view(rows, c * stack, out_wh[1], out_wh[0])


def _raw_single(frames, box, resized, x, y, out_wh, flip, stack, stat=None):
    from attention_based_tbn_amd._lib import call, ptr, stream_ptr
    n, H, W, c = frames.shape
    out = torch.empty((n // stack, c * stack, out_wh[1], out_wh[0]), device="cuda")
    mean, std = stat if stat else (None, None)
    call("tbn_frames_to_tensor", ptr(frames), n, H, W, c, *box, *resized, x, y, out_wh[0], out_wh[1], flip, stack,
         ptr(mean), ptr(std), 0 if mean is None else mean.numel(), 1, ptr(out), stream_ptr())
    return out


@pytest.mark.gpu
def test_raw_entry_writes_every_element_and_nothing_else():
    """guards before and after the output stay NaN, every element between them is written; odd sizes, a resize, more
    than one row tile, 100 Flow entries with pairs"""
    rng = np.random.RandomState(3)
    rgb = torch.from_numpy(rng.randint(0, 256, (3, 41, 57, 3)).astype(np.uint8)).cuda()
    flow = torch.from_numpy(rng.randint(0, 256, (10, 41, 57, 1)).astype(np.uint8)).cuda()
    stat = (torch.tensor([0.4, 0.5, 0.6]).cuda(), torch.tensor([0.2, 0.3, 0.4]).cuda())
    xs, ys = zip(*closed_form_windows(41, 57, (37, 23), [0, 1, 2, 3, 4]))
    for mirror in (0, 1, 2, 3):
        got = _raw_crops(rgb, (0, 0, 57, 41), (57, 41), xs, ys, (23, 37), mirror, 1, stat)
        assert got.shape == (15 * (2 if mirror >= 2 else 1), 3, 37, 23)
    got = _raw_crops(flow, (0, 0, 57, 41), (57, 41), xs, ys, (23, 37), 2, 10)
    assert got.shape == (10, 10, 37, 23)
    # a source box smaller than the frame, resized up, windows at the far corner of the resized box
    got = _raw_crops(rgb, (3, 2, 50, 35), (61, 47), (0, 61 - 23), (0, 47 - 37), (23, 37), 2, 1, stat)
    assert got.shape == (12, 3, 37, 23)


@pytest.mark.gpu
@pytest.mark.parametrize("resize", [False, True])
def test_one_window_agrees_with_the_single_window_entry(resize):
    rng = np.random.RandomState(4)
    stat = (torch.tensor([0.5]).cuda(), torch.tensor([0.226]).cuda())
    for c, stack, n in ((3, 1, 3), (1, 10, 20)):
        frames = torch.from_numpy(rng.randint(0, 256, (n, 41, 57, c)).astype(np.uint8)).cuda()
        box, resized = ((2, 1, 52, 38), (44, 35)) if resize else ((2, 1, 52, 38), (52, 38))
        for mirror in (0, 1):
            a = _raw_crops(frames, box, resized, (5,), (3,), (33, 29), mirror, stack, stat)
            b = _raw_single(frames, box, resized, 5, 3, (33, 29), mirror, stack, stat)
            assert torch.equal(a, b), (c, mirror)


@pytest.mark.gpu
def test_wide_windows_reach_the_second_column_trip():
    """output columns >= 256 are a thread's second trip: 40x700 frames, crop (16, 300)"""
    from attention_based_tbn_amd.core.dataset import DevicePipeline, FixedCrop, RandomHorizontalFlip
    rng = np.random.RandomState(6)
    frames = [rng.randint(0, 256, (40, 700, 3)).astype(np.uint8) for _ in range(2)]
    mean, std = [0.408, 0.459, 0.502], [0.229, 0.224, 0.225]
    for flip in (False, True):
        got = DevicePipeline("RGB", [FixedCrop((16, 300), [0, 2, 3], flip)], mean, std)(frames)
        want = otf.stack_totensor_normalize(np_fixed_crop(frames, (16, 300), [0, 2, 3], flip), "RGB", mean, std)
        assert np.array_equal(got.cpu().numpy(), want), flip
        # frames mirrored beforehand: the reference crops the mirrored frames
        got = DevicePipeline("RGB", [RandomHorizontalFlip(prob=1.0), FixedCrop((16, 300), [0, 2, 3], flip)], mean,
                             std)(frames)
        want = otf.stack_totensor_normalize(np_fixed_crop([np.fliplr(f) for f in frames], (16, 300), [0, 2, 3], flip),
                                            "RGB", mean, std)
        assert np.array_equal(got.cpu().numpy(), want), ("flip first", flip)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(256, 456), (240, 320)])
def test_ten_crop_pipeline_full_size_vs_numpy(hw):
    """get_transforms(test_crops=10) at the real sizes (Rescale 256 -> ten 224 crops); 240x320 frames take the resize"""
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import get_transforms
    cfg = load_config([])
    rng = np.random.RandomState(hw[1])
    tfs = get_transforms(cfg, ["RGB", "Flow"], "test", test_crops=10)
    for m, n_img in (("RGB", 3), ("Flow", 30)):
        node = cfg.data.rgb if m == "RGB" else cfg.data.flow
        frames = [rng.randint(0, 256, hw + ((3,) if m == "RGB" else ())).astype(np.uint8) for _ in range(n_img)]
        got = tfs[m](frames)
        imgs = np_fixed_crop(otf.rescale(frames, cfg.data.test_scale_size), cfg.data.test_crop_size, [0, 1, 2, 3, 4], True)
        want = otf.stack_totensor_normalize(imgs, m, list(node.mean), list(node.std))
        assert tuple(got.shape) == want.shape == (n_img * 10 // (10 if m == "Flow" else 1), 3 if m == "RGB" else 10, 224, 224)
        assert np.array_equal(got.cpu().numpy(), want), m


@pytest.mark.gpu
def test_test_crops_1_is_todays_pipeline_and_the_centre_window():
    from attention_based_tbn_amd.config import load_config
    from attention_based_tbn_amd.core.dataset import (CenterCrop, DevicePipeline, FixedCrop, Normalize, Rescale, Stack,
                                                      ToTensor, get_transforms)
    cfg = load_config(["data.test_scale_size=40", "data.test_crop_size=32"])
    rng = np.random.RandomState(8)
    for m, n_img in (("RGB", 2), ("Flow", 10)):
        node = cfg.data.rgb if m == "RGB" else cfg.data.flow
        frames = [rng.randint(0, 256, (57, 45) + ((3,) if m == "RGB" else ())).astype(np.uint8) for _ in range(n_img)]
        today = get_transforms(cfg, [m], "test")[m](frames)
        assert torch.equal(get_transforms(cfg, [m], "test", test_crops=1)[m](frames), today)
        want = otf.stack_totensor_normalize(otf.test_geometry(frames, 40, 32), m, list(node.mean), list(node.std))
        assert np.array_equal(today.cpu().numpy(), want)
        one = DevicePipeline(m, [Rescale(40), FixedCrop(32, [0])], list(node.mean), list(node.std))(frames)
        assert torch.equal(one, today)
        # the reference's own test composition (core/tools/test.py:139-152), CenterCrop
        ref_style = compose([Rescale(40), CenterCrop(32), Stack(m), ToTensor(), Normalize(node.mean, node.std)], frames)
        assert torch.equal(ref_style, today)
    # Audio: Stack + ToTensor(is_audio=True) is AudioToTensor
    spec = [rng.randn(256, 20).astype(np.float32) for _ in range(3)]
    a = compose([Stack("Audio"), ToTensor(is_audio=True)], spec)
    assert torch.equal(a, get_transforms(cfg, ["Audio"], "test")["Audio"](spec)) and a.shape == (3, 1, 256, 20)


@pytest.mark.gpu
def test_five_crop_scores_are_the_mean_of_the_single_window_runs():
    """RGB-only TBNModel in eval: the consensus over 5 x n rows is the mean of the five single-window consensuses;
    only the order of summation differs"""
    from oracle.fill import fill_state_dict
    from attention_based_tbn_amd.core.dataset import DevicePipeline, FixedCrop
    from attention_based_tbn_amd.core.models import build_model
    from tests.util import assert_close, load_case
    cfg, modality, meta, data, inp, target = load_case("cfg2_rgb_only")
    model, _, _ = build_model(cfg, modality, torch.device("cuda"))
    model.load_state_dict(fill_state_dict(model.state_dict(), meta["fill_seed"]))
    model.eval()
    size = inp["RGB"].shape[-1]
    rng = np.random.RandomState(9)
    frames = [rng.randint(0, 256, (size + 7, size + 21, 3)).astype(np.uint8) for _ in range(3)]
    mean, std = list(cfg.data.rgb.mean), list(cfg.data.rgb.std)

    def scores(locations):
        x = DevicePipeline("RGB", [FixedCrop(size, locations)], mean, std)(frames)
        with torch.no_grad():
            return {k: v.clone() for k, v in model({"RGB": x.unsqueeze(0)}).items()}
    five = scores([0, 1, 2, 3, 4])
    singles = [scores([loc]) for loc in range(5)]
    for k in five:
        want = torch.stack([s[k] for s in singles]).double().mean(0)
        assert five[k].shape == want.shape == (1, cfg.model.num_classes[k])
        assert_close(five[k], want, k)
        assert not torch.equal(singles[0][k], singles[1][k])        # the windows do differ
