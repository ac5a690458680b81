"""The convolutional half of the feature extractor: FPN encoder, merge layer and FPN decoder, one HIP launch per layer in inference.

A mirror, in this package's words, of the reference's `FPNEncoder`, `FPNDecoder_concat`, `Swish` and `Conv2d` (model/FPN.py:5-69,
88-128) and of the `merge_layer` expression of its constructor and `extract_features` (model/network.py:66, 182), for the
configuration GFNet builds: norm_type "BN".  Submodule and parameter names are the reference's, so the `encoder.*`, `decoder.*` and
`merge_layer.*` entries of a reference checkpoint load strictly:

    encoder   conv00 conv01 downsample1 conv10 conv11 downsample2 conv20 conv21 downsample3 conv30 conv31, each with
              .conv.weight  .bn.{weight,bias,running_mean,running_var,num_batches_tracked}
    decoder   out0 inner1 out1 inner2 out2 inner3 out3, each with .0.{weight,bias} (conv)  .1.* (BatchNorm)
    merge     0.{weight,bias}  1.*

Three paths over the same parameters:

  * in eval() on CUDA fp32 input with conv_impl "hip" (the default) every layer is ONE ops.conv2d_bn_act launch
    (csrc/fpn_conv.hip): BatchNorm's running statistics, its affine and the conv bias are folded into a per-channel scale and shift
    on the device at every forward (a few tiny torch ops, no host sync, nothing cached that load_state_dict could leave stale); the
    decoder's cat(interpolate(intra), convN1) and its `convN1 +` residual ride in the innerN launch, conv31 + merge(cat(conv31,
    side)) likewise, so neither the doubled map nor the concatenation is ever written.  No autograd on this path.
  * in train() on CUDA fp32 input with train_conv_impl "hip" (NOT the default) every layer is one ops.conv2d_bn_act_train call
    (csrc/fpn_conv_train.hip): convolution, the batch's own statistics, BatchNorm, activation and residual in HIP with a HIP backward.
    Autograd keeps the layer's inputs and ONE map per layer, the raw convolution output; the normalised map, the activation's mask
    or sigmoid and the concatenation are recomputed or never written.  The 2x upsample in front of innerN is F.interpolate
    (which differentiates it) and its result is passed as x0.  The BatchNorm buffers move as in the reference.  A conv bias in front
    of a batch-statistics BatchNorm (the decoder's and the merge layer's) gets EXACT zeros as its gradient: it cancels in u - mean,
    the true gradient is zero, and torch's autograd returns rounding noise around 1e-7 there.
  * train_conv_impl "hip_fused" (opt-in like "hip") is "hip" for every layer but the decoder's inner1..3: those pass the coarse
    map with up0=True, and the op interpolates it on the way in, in the forward and in the weight gradient, and gathers the coarse
    input gradient with the transposed upsample (ft_up2_adjoint_kernel).  The doubled map is then neither written, nor kept by
    autograd, nor differentiated by torch; still 19 calls of the op per forward.
  * everything else -- train() with train_conv_impl "torch" (the default), CPU tensors, other dtypes, conv_impl "torch" in eval():
    F.conv2d, BatchNorm, the activation, F.interpolate and torch.cat, as the reference writes them; differentiable, and the
    BatchNorm buffers move as in the reference.

The top-level module's conv_impl, train_conv_impl and conv_precision govern its children (run(x, hip, train_hip, half, tf32)).

conv_precision "fp32" (the default, all of the above) or "fp16": an opt-in fp16 CLASS of the first path, and of that path only.
Exactly where the fp32 HIP path runs -- eval(), CUDA, conv_impl "hip" -- every layer is then ONE ops.conv2d_bn_act_half launch
(csrc/fpn_conv_half.hip): the image and the merge layer's side map are cast to fp16 on entry, every map between layers is fp16 in
memory, the convolution is an implicit GEMM on the matrix core (fp16 products, fp32 sums and epilogue, one rounding per stored
value), and EVERY RETURNED MAP IS fp16 -- the dtype of the result differs from the default's.  A layer that class cannot run (Cout
no multiple of 8) raises NotImplementedError naming the layer.  train(), CPU tensors and conv_impl "torch" run what they run under
"fp32", in fp32, whatever conv_precision says.  The reference runs its FPN in fp32 outside autocast: "fp16" is this package's
option, not the reference's arithmetic.

conv_precision takes the values of ALL_CONV_PRECISIONS ("fp32", "fp16", "tf32"); CONV_PRECISIONS is the pair of them that governs
eval() alone and keeps its older value.

conv_precision "tf32": the reference's own class, opt-in, for BOTH HIP paths.  The reference runs its FPN in fp32 tensors with
cuDNN's TF32 convolutions (train.py:151 sets torch.backends.cudnn.allow_tf32, torch's default for convolutions): fp32 maps, the
operands of each product rounded, fp32 sums.  gfx950 has no TF32 matrix instruction, so the class is split-bf16 on the bf16 one, as
include/gfnet_hip.h states it once:

    the split of an fp32 value v: hi = bf16(v) to nearest even, lo = bf16(v - hi), lo = 0 where hi is not finite (an inf stays an inf);
    a product a b is a_hi b_hi + a_hi b_lo + a_lo b_hi, each exact in fp32 and summed in fp32 on the matrix core; a_lo b_lo is dropped;
    with up0 the interpolated value is computed in fp32 as today and then split; scale, shift, activation, residual and every map fp32.

The error against exact arithmetic is at most 3 * 2^-16 * sum |a| |b| per output before fp32 accumulation, against TF32's 2^-10.
Exactly where _use_hip is true every layer is ONE ops.conv2d_bn_act_tf32 launch (csrc/fpn_conv_tf32.hip), fp32 in and out; under
train_conv_impl "hip" and "hip_fused" every layer passes precision="tf32" to ops.conv2d_bn_act_train, which runs the forward
convolution, the stride-1 input gradient and the stride-1 weight gradient (without up0) in the class and leaves the stride-2 input
gradient and the stride-2 and up0 weight gradients on the fp32 kernels.  A layer whose Cout is not a multiple of 8 (GFNet builds none) runs the fp32 kernels silently in both modes.  Nothing
downstream changes: the maps, autograd's saved tensors and the BatchNorm passes are those of "fp32".  CPU tensors and the torch
paths run what they run under "fp32".
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

CONV_IMPLS = ("hip", "torch")
TRAIN_CONV_IMPLS = ("hip", "hip_fused", "torch")  # "hip_fused": "hip" with the decoder's 2x upsample inside the innerN op
# The values conv_precision takes are ALL_CONV_PRECISIONS: that is the tuple to validate against and to offer as choices.
# CONV_PRECISIONS is the older, shorter tuple kept under its name and value for callers that hold it: the classes that govern eval()
# ALONE ("fp16": fp16 maps and the matrix core on the eval() HIP path).  "tf32" (fp32 maps, split-bf16 operands on the matrix core)
# governs the eval() AND the train() HIP paths (module docstring)
CONV_PRECISIONS = ("fp32", "fp16")
ALL_CONV_PRECISIONS = CONV_PRECISIONS + ("tf32",)
LEAKY_SLOPE = 0.1  # FPN.py:127


def _check_impl(conv_impl):
    if conv_impl not in CONV_IMPLS:
        raise ValueError(f"conv_impl must be one of {CONV_IMPLS}, got {conv_impl!r}")
    return conv_impl


def _check_train_impl(train_conv_impl):
    if train_conv_impl not in TRAIN_CONV_IMPLS:
        raise ValueError(f"train_conv_impl must be one of {TRAIN_CONV_IMPLS}, got {train_conv_impl!r}")
    return train_conv_impl


def _check_precision(conv_precision):
    if conv_precision not in ALL_CONV_PRECISIONS:
        raise ValueError(f"conv_precision must be one of {ALL_CONV_PRECISIONS}, got {conv_precision!r}")
    return conv_precision


def _use_half(module, x):
    """The fp16 class: where the fp32 HIP path would run, on an fp32 or fp16 map (cast to fp16 on entry)."""
    _check_impl(module.conv_impl)
    return (_check_precision(module.conv_precision) == "fp16" and module.conv_impl == "hip" and not module.training and x.is_cuda
            and x.dtype in (torch.float32, torch.float16))


def _use_tf32(module):
    """The TF32 class: wherever a HIP path runs, eval() or train(), that path's convolutions in that class."""
    return _check_precision(module.conv_precision) == "tf32"


def _use_hip(module, x):
    _check_impl(module.conv_impl)
    return module.conv_impl == "hip" and not module.training and x.is_cuda and x.dtype == torch.float32


def _use_train_hip(module, x):
    _check_train_impl(module.train_conv_impl)
    return module.train_conv_impl in ("hip", "hip_fused") and module.training and x.is_cuda and x.dtype == torch.float32


def _fold(conv, bn):
    """(scale, shift) with bn(conv(x)) = conv_without_bias(x) * scale + shift in eval mode, as device tensors."""
    with torch.no_grad():
        if bn is None:
            scale = torch.ones_like(conv.weight[:, 0, 0, 0])
            return scale, (conv.bias if conv.bias is not None else torch.zeros_like(scale)).contiguous()
        scale = torch.rsqrt(bn.running_var + bn.eps)
        if bn.weight is not None:
            scale = scale * bn.weight
        shift = -bn.running_mean * scale
        if bn.bias is not None:
            shift = shift + bn.bias
        if conv.bias is not None:
            shift = shift + conv.bias * scale
        return scale.contiguous(), shift.contiguous()


def _check_conv(conv, switch):
    k = conv.kernel_size[0]
    if (conv.kernel_size != (k, k) or k not in (1, 3, 5, 7) or conv.padding != (k // 2, k // 2) or conv.stride not in ((1, 1), (2, 2))
            or conv.dilation != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros"):
        raise NotImplementedError(f"{switch}='hip' runs square kernels of 1, 3, 5 or 7 with padding k // 2, stride 1 or 2, no dilation "
                                  f"and no groups; got {conv}: construct with {switch}='torch'")


def _hip_train_layer(conv, bn, act, x0, x1=None, residual=None, up0=False, tf32=False):
    """One layer on the batch's own statistics through ops.conv2d_bn_act_train; where the layer upsamples x0 is the doubled map, or
    with up0 the coarse one."""
    _check_conv(conv, "train_conv_impl")
    if bn is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("train_conv_impl='hip' needs an affine BatchNorm2d that tracks its running statistics after every "
                                  "convolution: construct with train_conv_impl='torch'")
    x0, x1, residual = (None if t is None else t.contiguous() for t in (x0, x1, residual))
    return ops.conv2d_bn_act_train(x0, conv.weight.contiguous(), conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                   bn.num_batches_tracked, bn.momentum, bn.eps, x1=x1, residual=residual, stride=conv.stride[0], act=act,
                                   slope=LEAKY_SLOPE, up0=up0, precision="tf32" if tf32 else "fp32")


def _hip_layer(conv, bn, act, x0, x1=None, up0=False, residual=None, half=False, tf32=False):
    _check_conv(conv, "conv_impl")
    scale, shift = _fold(conv, bn)
    x0, x1, residual = (None if t is None else t.contiguous() for t in (x0, x1, residual))
    if half:
        if conv.out_channels % 8:
            raise NotImplementedError(f"conv_precision='fp16' runs layers whose output channels are a multiple of 8; got {conv}: "
                                      "construct with conv_precision='fp32'")
        return ops.conv2d_bn_act_half(x0, conv.weight.detach().contiguous(), scale.float(), shift.float(), x1=x1, up0=up0,
                                      residual=residual, stride=conv.stride[0], act=act, slope=LEAKY_SLOPE)
    if tf32 and conv.out_channels % 8 == 0:  # (any other layer runs the fp32 op: exact products lie within the class)
        return ops.conv2d_bn_act_tf32(x0, conv.weight.detach().contiguous(), scale, shift, x1=x1, up0=up0, residual=residual,
                                      stride=conv.stride[0], act=act, slope=LEAKY_SLOPE)
    return ops.conv2d_bn_act(x0, conv.weight.detach().contiguous(), scale, shift, x1=x1, up0=up0, residual=residual, stride=conv.stride[0],
                             act=act, slope=LEAKY_SLOPE)


def _up2(x):
    # FPN.py:59: the coarser map goes through interpolate in fp32 (float64, which only tests use, is left alone)
    return F.interpolate(x if x.dtype == torch.float64 else x.to(torch.float32), scale_factor=2, mode="bilinear", align_corners=False)


class Swish(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


class Conv2d(nn.Module):
    """FPN.py:95-134: convolution (no bias when a BatchNorm follows), BatchNorm, leaky ReLU 0.1.  norm_type defaults to "BN" here: the
    reference's "IN" (InstanceNorm, which GFNet never builds) raises NotImplementedError."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, relu=True, bn=True, bn_momentum=0.1, norm_type="BN",
                 conv_impl="hip", train_conv_impl="torch", conv_precision="fp32", **kwargs):
        super().__init__()
        self.conv_precision = _check_precision(conv_precision)
        if norm_type != "BN":
            raise NotImplementedError(f"Conv2d: norm_type = {norm_type!r} is not supported, only 'BN' (what GFNet builds)")
        self.conv_impl = _check_impl(conv_impl)
        self.train_conv_impl = _check_train_impl(train_conv_impl)
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)
        self.kernel_size = kernel_size
        self.stride = stride
        self.bn = nn.BatchNorm2d(out_channels, momentum=bn_momentum) if bn else None
        self.relu = relu

    def run(self, x, hip, train_hip=False, half=False, tf32=False):
        if hip:
            return _hip_layer(self.conv, self.bn, "leaky_relu" if self.relu else None, x.half() if half else x, half=half, tf32=tf32)
        if train_hip:
            return _hip_train_layer(self.conv, self.bn, "leaky_relu" if self.relu else None, x, tf32=tf32)
        y = self.conv(x)
        if self.bn is not None:
            y = self.bn(y)
        return F.leaky_relu(y, LEAKY_SLOPE, inplace=True) if self.relu else y

    def forward(self, x):
        half = _use_half(self, x)
        return self.run(x, half or _use_hip(self, x), _use_train_hip(self, x), half, _use_tf32(self))


class FPNEncoder(nn.Module):
    """FPN.py:5-36: images (B, 3, H, W) -> [conv01, conv11, conv21, conv31] at strides 1, 2, 4, 8 with feat_chs channels (fine to
    coarse).  H and W must be multiples of 8 (the reference fails later, inside the decoder's torch.cat)."""

    def __init__(self, feat_chs, norm_type="BN", conv_impl="hip", train_conv_impl="torch", conv_precision="fp32"):
        super().__init__()
        self.conv_precision = _check_precision(conv_precision)
        if norm_type != "BN":
            raise NotImplementedError(f"FPNEncoder: norm_type = {norm_type!r} is not supported, only 'BN' (what GFNet builds)")
        self.conv_impl = _check_impl(conv_impl)
        self.train_conv_impl = _check_train_impl(train_conv_impl)
        c = feat_chs
        kw = {"norm_type": norm_type, "conv_impl": conv_impl, "train_conv_impl": train_conv_impl, "conv_precision": conv_precision}
        self.conv00 = Conv2d(3, c[0], 7, 1, padding=3, **kw)
        self.conv01 = Conv2d(c[0], c[0], 5, 1, padding=2, **kw)

        self.downsample1 = Conv2d(c[0], c[1], 5, stride=2, padding=2, **kw)
        self.conv10 = Conv2d(c[1], c[1], 3, 1, padding=1, **kw)
        self.conv11 = Conv2d(c[1], c[1], 3, 1, padding=1, **kw)

        self.downsample2 = Conv2d(c[1], c[2], 5, stride=2, padding=2, **kw)
        self.conv20 = Conv2d(c[2], c[2], 3, 1, padding=1, **kw)
        self.conv21 = Conv2d(c[2], c[2], 3, 1, padding=1, **kw)

        self.downsample3 = Conv2d(c[2], c[3], 3, stride=2, padding=1, **kw)
        self.conv30 = Conv2d(c[3], c[3], 3, 1, padding=1, **kw)
        self.conv31 = Conv2d(c[3], c[3], 3, 1, padding=1, **kw)

    def forward(self, x):
        if x.dim() != 4 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"FPNEncoder: height and width must be multiples of 8, got an input of shape {tuple(x.shape)}")
        half = _use_half(self, x)  # (the image is cast to fp16 by the first layer's run, every later map already is)
        mode = (half or _use_hip(self, x), _use_train_hip(self, x), half, _use_tf32(self))
        conv01 = self.conv01.run(self.conv00.run(x, *mode), *mode)
        conv11 = self.conv11.run(self.conv10.run(self.downsample1.run(conv01, *mode), *mode), *mode)
        conv21 = self.conv21.run(self.conv20.run(self.downsample2.run(conv11, *mode), *mode), *mode)
        conv31 = self.conv31.run(self.conv30.run(self.downsample3.run(conv21, *mode), *mode), *mode)
        return [conv01, conv11, conv21, conv31]


def _head(seq):
    return seq[0], seq[1], "swish"


class merge_layer(nn.Sequential):
    """network.py:66, 182: `conv31 + Sequential(conv3x3(2 ch -> ch), BatchNorm, Swish)(cat(conv31, side))`, the addition included:
    forward(conv31, side) -> the merged stride-8 map."""

    def __init__(self, ch, conv_impl="hip", train_conv_impl="torch", conv_precision="fp32"):
        super().__init__(nn.Conv2d(2 * ch, ch, kernel_size=3, padding=1), nn.BatchNorm2d(ch), Swish())
        self.conv_precision = _check_precision(conv_precision)
        self.conv_impl = _check_impl(conv_impl)
        self.train_conv_impl = _check_train_impl(train_conv_impl)

    def forward(self, conv31, side):
        if conv31.shape != side.shape:
            raise ValueError(f"merge_layer: conv31 {tuple(conv31.shape)} and the side map {tuple(side.shape)} must have one shape")
        if _use_half(self, conv31) and _use_half(self, side):
            conv31 = conv31.half()
            return _hip_layer(*_head(self), conv31, x1=side.half(), residual=conv31, half=True)
        if _use_hip(self, conv31) and side.is_cuda and side.dtype == torch.float32:
            return _hip_layer(*_head(self), conv31, x1=side, residual=conv31, tf32=_use_tf32(self))
        if _use_train_hip(self, conv31) and side.is_cuda and side.dtype == torch.float32:
            return _hip_train_layer(*_head(self), conv31, x1=side, residual=conv31, tf32=_use_tf32(self))
        return conv31 + nn.Sequential.forward(self, torch.cat((conv31, side), dim=1))


class FPNDecoder_concat(nn.Module):
    """FPN.py:39-69: (conv01, conv11, conv21, conv31) -> [out0, out1, out2, out3] at strides 8, 4, 2, 1."""

    def __init__(self, feat_chs, conv_impl="hip", train_conv_impl="torch", conv_precision="fp32"):
        super().__init__()
        self.conv_precision = _check_precision(conv_precision)
        self.conv_impl = _check_impl(conv_impl)
        self.train_conv_impl = _check_train_impl(train_conv_impl)
        c = feat_chs

        def block(cin, cout, k):
            return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=k, padding=k // 2), nn.BatchNorm2d(cout), Swish())

        self.out0 = block(c[-1], c[-1], 1)

        self.inner1 = block(c[-1] + c[-2], c[-2], 3)
        self.out1 = block(c[-2], c[-2], 1)

        self.inner2 = block(c[-2] + c[-3], c[-3], 3)
        self.out2 = block(c[-3], c[-3], 1)

        self.inner3 = block(c[-3] + c[-4], c[-4], 3)
        self.out3 = block(c[-4], c[-4], 1)

    def forward(self, conv01, conv11, conv21, conv31):
        maps = (conv31, conv21, conv11, conv01)
        for coarse, fine in zip(maps, maps[1:]):
            if fine.shape[0] != coarse.shape[0] or tuple(fine.shape[2:]) != (2 * coarse.shape[2], 2 * coarse.shape[3]):
                raise ValueError(f"FPNDecoder_concat: every level must double the one below it, got {[tuple(m.shape) for m in maps]} "
                                 "(image heights and widths must be multiples of 8)")
        half = all(_use_half(self, m) for m in maps)
        if half:
            conv01, conv11, conv21, conv31 = (m.half() for m in (conv01, conv11, conv21, conv31))
            maps = (conv31, conv21, conv11, conv01)
        hip = half or (_use_hip(self, conv31) and all(m.is_cuda and m.dtype == torch.float32 for m in maps))
        th = _use_train_hip(self, conv31) and all(m.is_cuda and m.dtype == torch.float32 for m in maps)
        tf32 = _use_tf32(self)
        intra = conv31
        outs = []
        for inner, out, skip in ((None, self.out0, None), (self.inner1, self.out1, conv21), (self.inner2, self.out2, conv11),
                                 (self.inner3, self.out3, conv01)):
            if inner is not None:  # FPN.py:59: skip + inner(cat(interpolate(intra), skip))
                if hip:
                    intra = _hip_layer(*_head(inner), intra, x1=skip, up0=True, residual=skip, half=half, tf32=tf32)
                elif th and self.train_conv_impl == "hip_fused":  # the upsample inside the op, in both directions
                    intra = _hip_train_layer(*_head(inner), intra, x1=skip, residual=skip, up0=True, tf32=tf32)
                elif th:  # the doubled map from torch, which differentiates the upsample; still no concatenation
                    intra = _hip_train_layer(*_head(inner), _up2(intra), x1=skip, residual=skip, tf32=tf32)
                else:
                    intra = skip + inner(torch.cat((_up2(intra), skip), dim=1))
            outs.append(_hip_layer(*_head(out), intra, half=half, tf32=tf32) if hip
                        else _hip_train_layer(*_head(out), intra, tf32=tf32) if th else out(intra))
        return outs
