"""`create_dataloader(cfg, logger, modality, mode)` of the reference (`core/utils/create_dataloader.py:84-128`), returning a
`ClipLoader` over a device-side `Video_Dataset` instead of a `torch.utils.data.DataLoader`.

What differs from the DataLoader, on purpose:
  * a batch is made at once by `Video_Dataset.batch` (one decode and one transform launch per modality), not item by item
    and collated;
  * iteration is synchronous on the current stream: no background thread, no prefetch, no worker processes.  The decode
    pool of `decode_jpegs` is the only host parallelism, so `cfg.num_workers` is accepted and ignored;
  * train order is `torch.randperm(N)`, drawn once per `__iter__` from the global torch generator.  That is a seeded,
    reproducible shuffle, but it is NOT pinned to the draw of `torch.utils.data.RandomSampler` (which seeds a generator
    of its own from the global one first): the same `torch.manual_seed` gives another order than the reference's loader.
The last, shorter batch is kept, as with the DataLoader's default `drop_last=False`.
"""
import os

import torch

from ..dataset.dataset import Video_Dataset
from ..dataset.transform import get_transforms


class ClipLoader(object):
    """iterable over the batches of a `Video_Dataset`: `len()` = ceil(N / batch_size), `.dataset`, `.batch_size`"""

    def __init__(self, dataset, batch_size, shuffle=False):
        if batch_size < 1:
            raise ValueError(f"ClipLoader: batch_size {batch_size}")
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    def batches(self):
        """the index lists of one pass; with `shuffle` one `torch.randperm` draw from the global generator"""
        n = len(self.dataset)
        order = torch.randperm(n).tolist() if self.shuffle else list(range(n))
        return [order[i:i + self.batch_size] for i in range(0, n, self.batch_size)]

    def __iter__(self):
        for part in self.batches():
            yield self.dataset.batch(part)


def create_dataloader(cfg, logger, modality, mode="test", device="cuda"):
    """The annotation file, video list and batch size per mode follow the reference (:86-120); val reads the TRAIN
    annotation file filtered by the val video list, as there.  A relative `vid_list` path is taken from the directory
    above the `core` package, like the reference's; an empty one keeps every video."""
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
    dataset = Video_Dataset(cfg, vid_list, annotation_file, modality, transform=transforms, mode=mode, device=device)
    loader = ClipLoader(dataset, batch_size, shuffle=(mode == "train"))
    logger.info("Done.")
    logger.info("----------------------------------------------------------")
    return loader
