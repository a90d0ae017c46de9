from .sampler import SegmentSampler, frame_span, get_offsets  # noqa: F401
from .spectrogram import Spectrogram, stft_geometry, trim_audio, trim_audio_window  # noqa: F401
from .prior import attention_prior, gaussian_kernel  # noqa: F401
from .audio import AudioSegments, audio_windows, window_table  # noqa: F401
from .transform import (CenterCrop, DevicePipeline, FixedCrop, MultiScaleCrop, Normalize, RandomCrop,  # noqa: F401
                        RandomHorizontalFlip, Rescale, Stack, ToTensor, TransferTensorDict, get_transforms)
from .frames import FrameReader, decode_jpegs, jpeg_geometry  # noqa: F401
from .frames import decode_frames, decode_pngs, png_fallback_count, png_geometry  # noqa: F401
from .dataset import EpicVideoRecord, Video_Dataset, read_wav  # noqa: F401
from .audio_file import WavInfo, load_audio, wav_info  # noqa: F401
from .npz_file import NpzMember, load_npz_arrays, npz_chunk_index, npz_member  # noqa: F401
from .epic_class import EpicClasses  # noqa: F401
