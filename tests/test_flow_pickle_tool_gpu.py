"""preprocessing/create_epic_flow_pickle.py end to end on a small tree built from tests/golden/flow_frames.npz: the files the
reference's loop names, their arrays, what a second run keeps, what a damaged file and a missing JPEG cause."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIN = 5
ROWS = [(4, 20), (0, 14)]          # (start_frame, stop_frame): the second starts at 0 and overlaps the first


@pytest.fixture(scope="module")
def frames(golden_dir):
    with np.load(os.path.join(golden_dir, "flow_frames.npz")) as z:
        return {k: z[k].tobytes() for k in z.files}


@pytest.fixture()
def tree(tmp_path, frames):
    for uv in "uv":
        d = tmp_path / "flow" / "P01" / "P01_01" / uv
        d.mkdir(parents=True)
        for i in range(9):
            (d / "frame_{:010d}.jpg".format(i + 1)).write_bytes(frames[f"{uv}_{i}"])
    csv = tmp_path / "annotations.csv"
    csv.write_text("uid,participant_id,video_id,start_frame,stop_frame\n" +
                   "".join(f"{k},P01,P01_01,{a},{b}\n" for k, (a, b) in enumerate(ROWS)))
    return tmp_path


def _argv(tree, *more):
    return [str(tree / "annotations.csv"), str(tree / "flow"), "--out-dir", str(tree / "out"), "--win-len", str(WIN), *more]


def _reference_names():
    """the reference's loop (its lines 175-181), restated: the file of every idx of every row"""
    names = []
    for start_frame, stop_frame in ROWS:
        start = np.maximum(start_frame // 2, 1)
        end = np.maximum(stop_frame // 2, 2)
        names += ["frame_{:010d}.npz".format(idx - 1) for idx in np.arange(start, end + 1 - WIN)]
    return names


def _mtimes(d):
    return {p.name: p.stat().st_mtime_ns for p in d.iterdir()}


def test_the_tool_writes_the_reference_files_keeps_sound_ones_and_rewrites_a_damaged_one(tree, frames):
    from attention_based_tbn_amd.core.dataset.frames import decode_jpegs
    from attention_based_tbn_amd.preprocessing.create_epic_flow_pickle import main
    names = _reference_names()
    assert len(names) == 6 and len(set(names)) == 5          # the rows overlap: 5 files, one of them named twice
    written, kept = main(_argv(tree))
    out = tree / "out" / "flow_pickle" / "P01_01"
    assert sorted(p.name for p in out.iterdir()) == sorted(set(names))
    assert sorted(map(os.path.basename, written)) == sorted(set(names)) and len(kept) == 1
    planes = {uv: decode_jpegs([frames[f"{uv}_{i}"] for i in range(9)], gray=True).cpu().numpy() for uv in "uv"}
    for name in set(names):
        idx = int(name[6:16]) + 1
        want = np.concatenate([planes[uv][idx + i - 1] for i in range(WIN) for uv in "uv"], axis=2)
        with np.load(out / name) as z:
            assert z.files == ["flow"] and z["flow"].shape == (40, 56, 2 * WIN) and np.array_equal(z["flow"], want), name
    # a second run rewrites nothing
    before = _mtimes(out)
    written, kept = main(_argv(tree))
    assert written == [] and len(kept) == 6 and _mtimes(out) == before
    # a truncated file is rewritten, and only that one
    victim = out / sorted(set(names))[2]
    blob = victim.read_bytes()
    victim.write_bytes(blob[:len(blob) // 2])
    written, _ = main(_argv(tree))
    assert written == [str(victim)] and victim.read_bytes() == blob
    after = _mtimes(out)
    assert {n for n in before if before[n] != after[n]} == {victim.name}


def test_the_host_deflate_path_writes_files_with_the_same_arrays(tree):
    from attention_based_tbn_amd.preprocessing.create_epic_flow_pickle import main
    main(_argv(tree))
    out = tree / "out" / "flow_pickle" / "P01_01"
    device = {p.name: np.load(p)["flow"] for p in out.iterdir()}
    for p in out.iterdir():
        p.unlink()
    written, _ = main(_argv(tree, "--deflate", "host"))
    assert len(written) == 5
    for p in out.iterdir():
        assert np.array_equal(np.load(p)["flow"], device[p.name])


def test_a_missing_jpeg_raises_and_names_the_path(tree):
    from attention_based_tbn_amd.preprocessing.create_epic_flow_pickle import main
    gone = tree / "flow" / "P01" / "P01_01" / "v" / "frame_0000000006.jpg"
    gone.unlink()
    with pytest.raises(FileNotFoundError, match=str(gone)):
        main(_argv(tree))
    assert torch.cuda.is_available()
