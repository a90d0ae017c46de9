"""What the backbones composed from the stand-alone HIP operators (Resnet, VGG, BNInception_Audio) share: the knobs TBNModel
sets on every backbone, the per-unit state kept on the parameter containers, the conv + BatchNorm + ReLU unit and the refusal
of a CPU input.  ops_conv.py knows tensors only; everything here knows nn.Conv2d / nn.BatchNorm2d containers."""
from ... import ops_conv
from ..._lib import TbnHipError


class OpsBackbone:
    """mix-in beside nn.Module.  The knobs steer the backbone engine, which these backbones do not use: the stream knobs are
    accepted and ignored, the conv math modes other than the defaults are refused.  (Not here, on purpose: `plan_sync`,
    `grad_bucket_fn`, `_out_slot` -- TBNModel and DataParallel take their presence for the engine's.)"""
    use_aux_stream = use_branch_streams = stem_wgrad_last = False
    _conv_math, _conv_math_layers = "f32", "3x3"

    @property
    def conv_math(self):
        return self._conv_math

    @conv_math.setter
    def conv_math(self, value):
        if value != "f32":
            raise ValueError(f"{type(self).__name__}: conv_math {value!r} is not available (the split-bf16 modes cover the "
                             "BN-Inception engine only); \"f32\" is the only mode")
        self._conv_math = value

    @property
    def conv_math_layers(self):
        return self._conv_math_layers

    @conv_math_layers.setter
    def conv_math_layers(self, value):
        if value != "3x3":
            raise ValueError(f"{type(self).__name__}: conv_math_layers {value!r} is not available; \"3x3\" (the default) is "
                             "the only value")
        self._conv_math_layers = value

    def flip_weights_early(self):
        """no-op: the operator-level data gradients prepare their weights themselves"""

    def _need_gpu(self, input):
        if not input.is_cuda:
            raise TbnHipError(f"{type(self).__name__}: input is on the CPU; this backbone only runs on an MI355X via "
                              "libtbn_hip.so (no CPU fallback)")


def unit_state(conv, bn=None):
    """the unit's BnState, kept on the conv container so its weight / fold caches live from call to call; stride and pad are
    the container's, the running buffers are read anew at every call (module.to() replaces them)"""
    s = conv.__dict__.get("_tbn_state")
    if s is None:
        s = conv.__dict__["_tbn_state"] = ops_conv.BnState(conv.stride[0], conv.padding[0], None, None)
    if bn is not None:
        s.running_mean, s.running_var = bn.running_mean, bn.running_var
    return s


def count_batch(training, *bns):
    """what nn.BatchNorm2d.forward does to its counter in training"""
    if training:
        for bn in bns:
            bn.num_batches_tracked += 1


def conv_bn_relu(conv, bn, x, training):
    """relu(bn(conv(x) + bias)) of a container pair, NHWC in and out"""
    out = ops_conv.conv_bn_act(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv.stride[0],
                               conv.padding[0], relu=True, training=training, state=unit_state(conv, bn), bias=conv.bias)
    count_batch(training, bn)
    return out
