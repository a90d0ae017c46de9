"""`python -m attention_based_tbn_amd.preprocessing.create_epic_flow_pickle ANNOTATION_FILE ROOT_DIR [--out-dir DIR]
[--file-format frame_{:010d}.jpg] [--win-len 5] [--njobs 4] [--chunk-index]`

The reference's `preprocessing/create_epic_flow_pickle.py` with its arguments, its file layout and its index rule: for
every row of the annotation CSV (participant_id, video_id, start_frame, stop_frame) and every
idx in range(max(start_frame // 2, 1), max(stop_frame // 2, 2) + 1 - win_len), the u/v flow frames idx .. idx + win_len - 1
of ROOT_DIR/<participant>/<video>/{u,v}/ are stacked as (H, W, 2 * win_len) uint8 in the order u_i, v_i, u_i+1, ... and
written as member `flow` of OUT_DIR/flow_pickle/<video>/frame_{idx-1:010d}.npz -- the "flow pickle" that
`data.flow.read_flow_pickle=True` reads.

What differs is where the work happens.  Per annotation row every needed JPEG is decoded ONCE (`decode_jpegs(gray=True)`,
byte-identical to cv2.imread(path, 0); consecutive stacks share win_len - 1 pairs), the stacks are built on the device
and written in batches through `write_npz_files` (core/dataset/npz_file.py), whose `--deflate device` path compresses on
the device (csrc/deflate.hip) and whose `--deflate host` path is zlib level 6 in the same container, as
np.savez_compressed.  `--chunk-index` (device path only, off by default) records in every file where the 32-KB chunks of its
stream end, so that `load_npz_arrays` inflates it one wavefront per chunk; np.load reads such a file as any other.  An existing file is kept when it passes an integrity check -- the device inflates it and checks
its CRC-32 (`tbn_inflate_batch` status 0); np.load judges what the device path refuses -- and rewritten when it fails.
A missing JPEG raises FileNotFoundError with its path (the reference asserts).  `--njobs` sizes the JPEG reader's host
threads; there are no worker processes.
"""
import argparse
import csv
import io
import os
import sys
import zipfile

import numpy as np

BATCH = 96             # stacks per write_npz_files / integrity-check call
DEFAULT_DEFLATE = "device"


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="dump epic kitchens flow images into pickle files")
    parser.add_argument("annotation_file", type=str, help="<path_to_epic_kitchens>/annotations/<annotation_file>.csv")
    parser.add_argument("root_dir", type=str,
                        help="<path_to_epic_kitchens>/EPIC_KITCHENS_2018/frames_rgb_flow/flow/<train or test>")
    parser.add_argument("--out-dir", dest="out_dir", type=str, default="./epic/flow", help="path to save output files")
    parser.add_argument("--file-format", dest="file_format", type=str, default="frame_{:010d}.jpg",
                        help="naming format of image files")
    parser.add_argument("--win-len", dest="win_len", type=int, default=5, help="number of flow frames to read")
    parser.add_argument("--njobs", dest="njobs", type=int, default=4, help="host threads of the JPEG reader")
    parser.add_argument("--deflate", dest="deflate", choices=("device", "host"), default=DEFAULT_DEFLATE,
                        help="where the .npz members are compressed")
    parser.add_argument("--device", dest="device", type=str, default="cuda", help="device that decodes, stacks and checks")
    parser.add_argument("--chunk-index", dest="chunk_index", action="store_true",
                        help="record the chunk index in every file written (needs --deflate device)")
    return parser.parse_args(argv)


def stack_indices(start_frame, stop_frame, win_len):
    """the reference's index rule (its lines 175-181): the first flow frame of every stack of one annotation row"""
    start = max(int(start_frame) // 2, 1)
    end = max(int(stop_frame) // 2, 2)
    return range(start, end + 1 - win_len)


def _np_load_ok(blob):
    try:
        with np.load(io.BytesIO(blob)) as data:
            _ = data["flow"]
        return True
    except Exception:
        return False


def integrity_check(paths, device="cuda"):
    """-> per file: True when its `flow` member inflates completely and its CRC-32 holds.  The device judges every file
    whose record it takes (`npz_member`, one `tbn_inflate_batch` call per shape); np.load judges the others and those
    the device refuses."""
    from ..core.dataset.npz_file import load_npz_arrays, npz_member
    blobs, ok, groups = [], [], {}
    for i, p in enumerate(paths):
        with open(p, "rb") as f:
            blobs.append(f.read())
        try:
            rec = npz_member(blobs[i])
        except zipfile.BadZipFile:
            ok.append(False)
            continue
        ok.append(None)
        if rec.host:
            ok[i] = _np_load_ok(blobs[i])
        else:
            groups.setdefault(rec.shape, []).append((i, rec))
    for shape, members in groups.items():
        # a member the device refuses comes back with a non-zero status; its slot's content is not looked at here
        _, statuses = load_npz_arrays([blobs[i] for i, _ in members], records=[r for _, r in members], device=device,
                                      host_read=lambda k: np.zeros(shape, np.uint8))
        for (i, _), s in zip(members, statuses):
            ok[i] = True if s == 0 else _np_load_ok(blobs[i])
    return ok


def _read(path):
    if not os.path.exists(path):
        raise FileNotFoundError("{} file does not exist".format(path))
    with open(path, "rb") as f:
        return f.read()


def save_images_to_pickle(record, root_dir, out_dir, win_len, file_format, njobs, deflate, device, chunk_index=False):
    """one annotation row -> (written paths, kept paths)"""
    import torch

    from ..core.dataset.frames import decode_frames
    from ..core.dataset.npz_file import write_npz_files
    vid_id = record["video_id"]
    vid_path = os.path.join(root_dir, record["participant_id"], vid_id)
    o_dir = os.path.join(out_dir, "flow_pickle", vid_id)
    os.makedirs(o_dir, exist_ok=True)
    indices = list(stack_indices(record["start_frame"], record["stop_frame"], win_len))
    out_files = [os.path.join(o_dir, os.path.splitext(file_format.format(idx - 1))[0] + ".npz") for idx in indices]
    # which files are there and sound
    present = [k for k, f in enumerate(out_files) if os.path.exists(f)]
    sound = set()
    for at in range(0, len(present), BATCH):
        part = present[at:at + BATCH]
        for k, good in zip(part, integrity_check([out_files[k] for k in part], device)):
            if good:
                sound.add(k)
            else:
                print("{} is corrupted. Overwriting file.".format(out_files[k]))
    todo = [k for k in range(len(indices)) if k not in sound]
    kept = [out_files[k] for k in sorted(sound)]
    if not todo:
        return [], kept
    # every frame the missing stacks need, decoded once: u frames, then v frames, in one batch
    frames = sorted(set(indices[k] + i for k in todo for i in range(win_len)))
    blobs = [_read(os.path.join(vid_path, uv, file_format.format(f))) for uv in ("u", "v") for f in frames]
    planes = decode_frames(blobs, gray=True, device=device, threads=max(1, min(16, njobs)))       # (2 F, H, W, 1)
    F = len(frames)
    pairs = torch.cat((planes[:F], planes[F:]), dim=3)                                            # (F, H, W, 2): u_f, v_f
    slot = {f: j for j, f in enumerate(frames)}
    written = []
    for at in range(0, len(todo), BATCH):
        part = todo[at:at + BATCH]
        rows = torch.tensor([[slot[indices[k] + i] for i in range(win_len)] for k in part], device=pairs.device)
        stacks = pairs[rows]                                                                      # (n, win, H, W, 2)
        stacks = stacks.permute(0, 2, 3, 1, 4).reshape(len(part), pairs.shape[1], pairs.shape[2], 2 * win_len).contiguous()
        paths = [out_files[k] for k in part]
        write_npz_files(paths, stacks, "flow", deflate=deflate, chunk_index=chunk_index)
        written += paths
    return written, kept


def main(argv=None):
    """-> (written .npz paths, kept .npz paths), each in the order of the annotation rows"""
    args = argv if isinstance(argv, argparse.Namespace) else parse_args(argv)
    with open(args.annotation_file, newline="") as f:
        annotations = list(csv.DictReader(f))
    participants = sorted(set(r["participant_id"] for r in annotations))
    print("Processing {} video annotations for {} participants".format(len(annotations), len(participants)))
    print("----------------------------------------------------------")
    written, kept = [], []
    for record in annotations:
        w, k = save_images_to_pickle(record, args.root_dir, args.out_dir, args.win_len, args.file_format, args.njobs,
                                     args.deflate, args.device, chunk_index=getattr(args, "chunk_index", False))
        written += w
        kept += k
    print("Done: {} files written, {} kept".format(len(written), len(kept)))
    print("----------------------------------------------------------")
    return written, kept


if __name__ == "__main__":
    main()
    sys.exit(0)
