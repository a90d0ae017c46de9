# same export list as reference core/models/__init__.py:1-14 (the VGG backbone is out of scope)
from .attention import PositionalEncoding, MultiheadedAttention, UniModalAttention, PrototypeAttention
from .bn_inception import bninception, BNInception
from .bn_inception_audio import BNInception_Audio
from .dataparallel import DataParallel
from .model_builder import build_model
from .model import TBNModel, Fusion, Classifier
from .resnet import Resnet
from .contrast_loss import ContrastLoss
