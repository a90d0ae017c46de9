"""`python -m attention_based_tbn_amd.preprocessing.create_audio_pickle AUDIO_DIR [--sr 24000] [--out-dir DIR] [--ext wav]`

The reference's `preprocessing/create_audio_pickle.py` with its arguments: every audio file under AUDIO_DIR becomes one
`<name>.npy` of mono float32 samples at `--sr`, the "audio pickle" that `data.audio.read_audio_pickle=True` reads.  The
waveform comes from `load_audio` (decode, downmix and resampling on the device), not from librosa.

Deliberate deviation: a file that cannot be read is listed as rejected and NOT written.  The reference goes on to save
the previous file's samples under the failed file's name.
"""
import argparse
import os
import sys

import numpy as np


def parse_args(argv=None):
    here = os.path.dirname(os.path.realpath(__file__))
    parser = argparse.ArgumentParser(description="write the waveform of every audio file as a float32 .npy file")
    parser.add_argument("audio_dir", type=str, help="directory of the audio files")
    parser.add_argument("--sr", dest="sr", type=int, default=24000, help="sampling rate of the written waveforms")
    parser.add_argument("--out-dir", dest="out_dir", type=str, default=os.path.join(here, "audio_pickle"),
                        help="directory the .npy files are written to")
    parser.add_argument("--ext", dest="ext", type=str, default="wav", help="extension of the audio files")
    parser.add_argument("--device", dest="device", type=str, default="cuda", help="device that decodes and resamples")
    return parser.parse_args(argv)


def main(args):
    """-> (written .npy paths, rejected file names)"""
    from ..core.dataset.audio_file import load_audio
    if not os.path.isdir(args.audio_dir):
        raise SystemExit("Audio path {} does not exist".format(args.audio_dir))
    os.makedirs(args.out_dir, exist_ok=True)
    written, rejected = [], []
    print("Processing audio files ...")
    for folder, _, files in os.walk(args.audio_dir):
        for name in sorted(files):
            if not name.endswith(args.ext):
                continue
            try:
                sample = load_audio(os.path.join(folder, name), args.sr, device=args.device).cpu().numpy()
            except Exception as e:
                print("Failed to read audio file {} with error {}".format(name, e))
                rejected.append(name)
                continue
            out = os.path.join(args.out_dir, os.path.splitext(name)[0] + ".npy")
            np.save(out, sample)
            written.append(out)
    print("Finished creating numpy files.")
    print("----------------------------------------------------------")
    if rejected:
        print("List of rejected files: {}".format(rejected))
    return written, rejected


if __name__ == "__main__":
    main(parse_args())
    sys.exit(0)
