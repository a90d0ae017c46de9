# same export list as reference core/models/__init__.py:1-14 (VGG is exported; model.arch = "vgg" is not wired into
# TBNModel / build_model yet: DESIGN section 4d)
from .attention import PositionalEncoding, MultiheadedAttention, UniModalAttention, PrototypeAttention
from .bn_inception import bninception, BNInception
from .bn_inception_audio import BNInception_Audio
from .dataparallel import DataParallel
from .model_builder import build_model
from .model import TBNModel, Fusion, Classifier
from .resnet import Resnet
from .vgg import VGG
from .contrast_loss import ContrastLoss
