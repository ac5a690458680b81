"""Hot-path counterpart of the reference's model/network.py.

What is kept: the names and call signatures a caller of the reference sees --
`GFNet(conf, ...)` with `forward / match / sample / corr_volume / pos_embed`, and `ConvRefiner`
with the reference's parameter layout (`block1`, `hidden_blocks`, `out_conv`, `disp_emb`), so a
reference checkpoint's `conv_refiner.*` tensors load unchanged and `estimation.demo_estimation` /
`test.py` can drive this class.

What is different: every step between the feature pyramids and the sampled matches runs in the
gfx950 kernels of csrc/ (through gfnet_amd.ops): global correlation + soft-argmax, the refiner's
two gathers + displacement embedding + local correlation (written straight into the concat
buffer), the flow update, the inter-scale resize, match() post-processing, the KDE of sample().
The DINOv2 / cross-attention / FPN backbone is NOT part of this package (BASELINE north_star: "host
code stays PyTorch-ROCm for the FPN/transformer backbone"): pass it in as `backbone=`, a callable
`backbone(images, upsample) -> (pyramid_A, pyramid_B)` with the dict layout of
GFNet.extract_features (model/network.py:156-201), or feed pyramids directly to
`forward_pyramids` / `match_pyramids`.  The refiner's depthwise/pointwise conv stack
(model/network.py:560-563) runs on csrc/conv_stack.hip / conv_stack_half.hip / conv_stack_bf16.hip in eval mode (SURVEY 8(f) N1;
`conv_precision`: "fp32" exact fp32 products, "fp16" fp16 1x1 operands, "amp" the class the reference's amp=True refiners run in
under torch.autocast -- fp16 maps between the blocks --, "bf16" the same under amp_dtype=torch.bfloat16: bf16 maps and operands,
for a model trained in that class).  Training mode keeps the nn modules by default (BatchNorm uses batch statistics
there); with `train_conv_impl = "hip"` on a refiner its nine blocks run on csrc/conv_stack_train.hip instead (ops.conv_block_train:
batch-statistic forward, running-buffer update and backward in HIP) in the fp32 class, and with `train_conv_impl = "hip_amp"` on
an amp=True refiner on csrc/conv_stack_train_half.hip (ops.conv_block_train_amp) in the class the reference trains in: fp16 maps
between the blocks, fp16 operands on the matrix core, fp32 sums, parameters and parameter gradients, overflow to inf for the loss
scaler; with `train_conv_impl = "hip_bf16"` on an amp=True, amp_dtype=torch.bfloat16 refiner on csrc/conv_stack_train_bf16.hip
(ops.conv_block_train_bf16): the same with bf16 maps and operands, fp32's exponent range and no need for a loss scale.  GroupNorm or
other norm types, non-depthwise blocks and symmetric batches beyond what the nn path does are out of scope
and keep the modules.  Either way the refiner input is assembled with the same HIP launch as inference, which has a HIP backward
(ops.refiner_input; csrc/refiner_input_bwd.hip).  Refiners with sample_mode "nearest" / "bicubic" train through differentiable
torch ops instead.

Training (`model.train()`, grad mode on, pyramids or parameters that require grad): forward_pyramids returns flows and
certainties with an autograd graph, as the reference's forward does (network.py:230-281).  The scale-16 global match is
differentiable with respect to both feature maps (ops.corr_softargmax: backward in csrc/corr_softargmax_bwd.hip, which never
writes the volume), every flow update passes its gradient to the previous flow, the refiner's outputs and the certainty
(ops.flow_update), and the refiner input (ops.refiner_input) passes its gradient to both feature maps, the flow and disp_emb --
also when only the flow asks for one.  Detached as in the reference:
the resize between scales (network.py:271-281) and the local correlation's feature1 / flow (utils/local_correlation.py:54).
Calls without grad (inference, bench.py) take the plain launches: no extra work.
"""
import math
import os

import torch
import torch.nn as nn

from .. import ops
from ..utils.kde import kde

SCALES = ("16", "8", "4", "2", "1")


class ConvRefiner(nn.Module):
    """Per-scale refiner (reference: model/network.py:444-564).

    forward(num_grid, x, y, flow, scale_factor=1, logits=None) -> (delta_flow, delta_certainty,
    local_corr).  Input assembly (network.py:533-558) and, in eval mode, the conv stack
    (network.py:560-563) run in HIP; training mode keeps the nn modules unless `train_conv_impl`
    is "hip" (fp32 class, csrc/conv_stack_train.hip), "hip_amp" (fp16 autocast class, csrc/conv_stack_train_half.hip) or "hip_bf16"
    (bf16 autocast class on a refiner with amp_dtype=torch.bfloat16, csrc/conv_stack_train_bf16.hip).
    """

    def __init__(self, in_dim=6, hidden_dim=16, out_dim=2, dw=False, kernel_size=5, hidden_blocks=3,
                 displacement_emb=None, displacement_emb_dim=None, local_corr_num=None, corr_in_other=None,
                 no_im_B_fm=False, amp=False, concat_logits=False, use_bias_block_1=True, use_cosine_corr=False,
                 disable_local_corr_grad=False, is_classifier=False, sample_mode="bilinear", norm_type=nn.BatchNorm2d,
                 bn_momentum=0.1, amp_dtype=torch.float16):
        super().__init__()
        if sample_mode not in ("bilinear", "nearest", "bicubic"):
            # the reference hands it to F.grid_sample (network.py:537, 547) and local_correlation (:553-554), zeros padding
            raise ValueError(f"sample_mode must be 'bilinear', 'nearest' or 'bicubic', got {sample_mode!r}")
        # the reference stores these flags (network.py:496-501) and its forward (network.py:533-564) never reads any of them: they are
        # kept the same way -- attributes without effect -- so that a constructor call written for the reference behaves identically
        # here (rounds 1-4 raised NotImplementedError for them; VERDICT r4 "missing" 5)
        self.no_im_B_fm = no_im_B_fm
        self.concat_logits = concat_logits
        self.use_cosine_corr = use_cosine_corr
        self.disable_local_corr_grad = disable_local_corr_grad
        self.is_classifier = is_classifier
        self.bn_momentum = bn_momentum

        def block(cin, cout, bias=True):
            groups = cin if dw else 1
            if dw and cout % cin:
                raise ValueError("depthwise block needs out_dim divisible by in_dim")
            norm = norm_type(cout, momentum=bn_momentum) if norm_type is nn.BatchNorm2d else norm_type(num_channels=cout)
            return nn.Sequential(nn.Conv2d(cin, cout, kernel_size, 1, kernel_size // 2, groups=groups, bias=bias), norm,
                                 nn.ReLU(inplace=True), nn.Conv2d(cout, cout, 1, 1, 0))

        self.block1 = block(in_dim, hidden_dim, bias=use_bias_block_1)
        self.hidden_blocks = nn.Sequential(*[block(hidden_dim, hidden_dim) for _ in range(hidden_blocks)])
        self.out_conv = nn.Conv2d(hidden_dim, out_dim, 1, 1, 0)
        self.has_displacement_emb = bool(displacement_emb)
        if self.has_displacement_emb:
            self.disp_emb = nn.Conv2d(2, displacement_emb_dim, 1, 1, 0)
        self.local_corr_radius = local_corr_num
        self.local_corr_num = local_corr_num
        self.corr_in_other = corr_in_other
        self.amp = amp
        self.amp_dtype = amp_dtype
        self.sample_mode = sample_mode
        # "hip": eval-mode conv stack on csrc/conv_stack.hip (fp32, BatchNorm folded); "torch": nn modules
        # under autocast as in the reference (always used in training mode)
        self.conv_impl = "hip"
        # 1x1 conv operands on the HIP path: "fp32" (exact fp32 products, the CPU reference's class) or "fp16"
        # (operands rounded to fp16, fp32 accumulation: the autocast class the reference runs these refiners in on GPU); "amp": fp16
        # operands and fp16 maps between the blocks; "bf16": the same with bf16 operands and maps (csrc/conv_stack_bf16.hip), the
        # class to evaluate a bf16-trained model in -- nothing is held inside fp16's range, and no fp16 kernel ever runs in it
        self.conv_precision = "fp32"
        # training mode: "torch" keeps the nn modules (the default); "hip" runs block1 + hidden_blocks through
        # ops.conv_block_train where _hip_train_stack_supported() holds, "hip_amp" through ops.conv_block_train_amp (fp16 maps, the
        # class of an amp=True refiner under fp16 autocast) where _hip_amp_train_stack_supported() holds, "hip_bf16" through
        # ops.conv_block_train_bf16 (bf16 maps, amp=True with amp_dtype=torch.bfloat16) where _hip_bf16_train_stack_supported()
        # holds; the modules otherwise
        self.train_conv_impl = "torch"
        self.fold_out_conv = True  # multiply out_conv into the last block's 1x1 conv (see folded_stack)

    supports_reuse_d = True  # forward(..., reuse_d=): see GFNet.forward_pyramids

    def may_reuse_d(self, x, y, flow):
        """The previous iteration's concat tensor may be overwritten in place (through raw pointers: autograd's version counter
        never sees the write) only when it cannot sit in an autograd graph: block1 saves `d` for its weight gradients whenever
        grad mode is on and anything upstream or in this refiner asks for gradients."""
        if not torch.is_grad_enabled():
            return True
        return not (x.requires_grad or y.requires_grad or flow.requires_grad or any(p.requires_grad for p in self.parameters()))

    def assemble(self, num_grid, x, y, flow, scale_factor=1, reuse=None):
        """d = cat(grid_feature, x_hat, disp_emb, local_corr) (network.py:555) and the local_corr view.
        reuse: the d of the previous iteration at this scale (same x, same grid): its grid_feature planes are kept."""
        if not self.has_displacement_emb:
            raise NotImplementedError("refiners without displacement embedding are not used by GFNet")
        c = x.shape[1]
        dd = self.disp_emb.weight.shape[0]
        use_corr = bool(self.corr_in_other)
        emb = self.disp_emb
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or y.requires_grad or flow.requires_grad or
                                                  emb.weight.requires_grad or emb.bias.requires_grad)
        if needs_grad and self.sample_mode != "bilinear":
            return self._assemble_autograd(num_grid, x, y, flow, scale_factor)
        d = ops.refiner_input(num_grid, x, y, flow, self.disp_emb.weight, self.disp_emb.bias,
                              self.local_corr_radius if use_corr else 0, scale_factor=scale_factor, corr_in_other=use_corr, reuse=reuse,
                              sample_mode=self.sample_mode)
        return d, (d[:, 2 * c + dd:] if use_corr else None)

    def _assemble_autograd(self, num_grid, x, y, flow, scale_factor):
        """The same tensor from differentiable torch ops (network.py:537-555), for training with sample_mode "nearest" or
        "bicubic" (bilinear refiners train through ops.refiner_input's HIP backward): gradients reach the backbone
        features through both grid_samples, disp_emb's parameters, and feature0 of the local correlation (through the HIP
        backward gfn_local_corr_mode_bwd_f0; the reference samples feature1 under no_grad, utils/local_correlation.py:54-60).
        Only plain (non-symmetric) batches: training concatenates the pyramids itself."""
        import torch.nn.functional as F

        from ..utils.local_correlation import local_correlation

        b, c, hs, ws = x.shape
        G = int(num_grid)
        if flow.shape[0] != b:
            raise NotImplementedError("training-mode refiner input needs a plain batch (flow and features of equal batch size)")
        x, y, flow = x.float(), y.float(), flow.float()
        x_hat = F.grid_sample(y, flow.permute(0, 2, 3, 1), align_corners=False, mode=self.sample_mode)        # :537
        lin = torch.linspace(-1 + 1 / G, 1 - 1 / G, G, device=x.device)
        gy, gx = torch.meshgrid(lin, lin, indexing="ij")
        coords = torch.stack((gx, gy))[None].expand(b, 2, G, G)                                                 # :539-546
        grid_feature = F.grid_sample(x, coords.permute(0, 2, 3, 1), align_corners=False, mode=self.sample_mode)  # :547
        emb = self.disp_emb(40 / 32 * scale_factor * (flow - coords))                                           # :548-549
        parts = [grid_feature, x_hat, emb]
        lc = None
        if self.corr_in_other:
            lc = local_correlation((b, c, hs, ws), grid_feature, y, local_radius=self.local_corr_radius, num_grid=G, flow=flow,
                                   sample_mode=self.sample_mode)                                                 # :553-554
            parts.append(lc)
        return torch.cat(parts, dim=1), lc

    # ---- conv stack in HIP (eval mode): BatchNorm folded, fp32 (csrc/conv_stack.hip) ----------------
    def _hip_stack_supported(self):
        if self.training or self.conv_impl != "hip":
            return False
        for blk in [self.block1] + list(self.hidden_blocks):
            conv, norm, _, pw = blk
            if not isinstance(norm, nn.BatchNorm2d) or conv.groups != conv.in_channels or conv.out_channels != conv.in_channels \
                    or conv.kernel_size != (5, 5) or pw.in_channels != conv.out_channels:
                return False
        return True

    def _train_blocks_supported(self, d):
        """What both HIP training stacks need of the input and the modules: an fp32 CUDA map on a square grid, depthwise blocks whose
        norm is an affine BatchNorm2d that tracks running statistics with a float momentum, fp32 parameters."""
        if d.dim() != 4 or d.shape[-1] != d.shape[-2] or d.dtype != torch.float32 or not d.is_cuda:
            return False
        for blk in [self.block1] + list(self.hidden_blocks):
            conv, norm, _, pw = blk
            if not isinstance(norm, nn.BatchNorm2d) or conv.groups != conv.in_channels or conv.out_channels != conv.in_channels \
                    or conv.kernel_size != (5, 5) or pw.in_channels != conv.out_channels:
                return False
            if not norm.affine or not norm.track_running_stats or not isinstance(norm.momentum, float) or norm.running_mean is None:
                return False
            if any(p.dtype != torch.float32 for p in blk.parameters()):
                return False
        return True

    def _hip_train_stack_supported(self, d):
        """Training mode on csrc/conv_stack_train.hip: opt-in (`train_conv_impl = "hip"`), the fp32 class, depthwise blocks whose
        norm is an affine BatchNorm2d that tracks running statistics with a float momentum; anything else keeps the modules."""
        if not self.training or self.train_conv_impl != "hip" or self.conv_precision != "fp32":
            return False
        return self._train_blocks_supported(d)

    def _hip_amp_train_stack_supported(self, d):
        """Training mode on csrc/conv_stack_train_half.hip: opt-in (`train_conv_impl = "hip_amp"`) on a refiner that the modules would
        run under fp16 autocast (amp set, amp_dtype float16), same structure as "hip"; conv_precision, an eval-mode setting, is not
        consulted.  Anything else keeps the modules under autocast."""
        if not self.training or self.train_conv_impl != "hip_amp" or not self.amp or self.amp_dtype is not torch.float16:
            return False
        return self._train_blocks_supported(d)

    def _hip_bf16_train_stack_supported(self, d):
        """Training mode on csrc/conv_stack_train_bf16.hip: opt-in (`train_conv_impl = "hip_bf16"`) on a refiner that the modules would
        run under bf16 autocast (amp set, amp_dtype bfloat16), same structure as "hip".  Anything else -- an fp16 refiner with this
        switch, a bf16 refiner with "hip_amp" -- keeps the modules under autocast."""
        if not self.training or self.train_conv_impl != "hip_bf16" or not self.amp or self.amp_dtype is not torch.bfloat16:
            return False
        return self._train_blocks_supported(d)

    def _train_stack_hip(self, d, amp=False):
        """hidden_blocks(block1(d)) in training mode, network.py:560-562, one ops.conv_block_train per block (amp=True: one
        ops.conv_block_train_amp, amp=torch.bfloat16: one ops.conv_block_train_bf16; the first reads the fp32 d, the others the
        16-bit map before them)"""
        block = ops.conv_block_train_bf16 if amp is torch.bfloat16 else ops.conv_block_train_amp if amp else ops.conv_block_train
        h = d
        for conv, norm, _, pw in [self.block1] + list(self.hidden_blocks):
            h = block(h, conv.weight, conv.bias, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                      norm.num_batches_tracked, norm.momentum, norm.eps, pw.weight, pw.bias)
        return h

    def folded_stack(self, bf16=False):
        """Per block the packed parameters of ops.conv_block (eval-mode BatchNorm folded to
        y = x*alpha + beta in float64); cached until a parameter or running statistic changes.
        bf16: packed for ops.conv_block_bf16 (the 16-bit sections of a block rounded to bf16) instead of for ops.conv_block /
        ops.conv_block_half (fp16); which of the two is part of the cache key.
        out_conv follows the last block's 1x1 conv with nothing in between (network.py:487,563), so the
        two linear maps are multiplied out in float64 (W = W_out W_pw, b = W_out b_pw + b_out): the last
        block writes the 3 output channels directly instead of C channels that out_conv re-reads."""
        blocks = [self.block1] + list(self.hidden_blocks)
        key = tuple(t._version for blk in blocks for t in list(blk.parameters()) + list(blk.buffers())) + \
            tuple(p._version for p in self.out_conv.parameters()) + (str(self.out_conv.weight.device), self.fold_out_conv, "bf16" if bf16 else "fp16")
        if getattr(self, "_fold_key", None) == key:
            return self._fold
        fold = []
        with torch.no_grad():
            oc = self.out_conv
            ow = oc.weight.float().reshape(oc.out_channels, oc.in_channels).contiguous()
            ob = oc.bias.float().contiguous()
            pack = ops.conv_block_pack_bf16 if bf16 else ops.conv_block_pack
            for n, (conv, norm, _, pw) in enumerate(blocks):
                alpha = (norm.weight.double() / torch.sqrt(norm.running_var.double() + norm.eps)).float()
                beta = (norm.bias.double() - norm.running_mean.double() * alpha.double()).float()
                pw_w, pw_b = pw.weight.reshape(pw.out_channels, -1), pw.bias
                if self.fold_out_conv and n == len(blocks) - 1:
                    pw_b = (ow.double() @ pw_b.double() + ob.double()).float()
                    pw_w = (ow.double() @ pw_w.double()).float()
                fold.append((pack(conv.weight, conv.bias, alpha, beta, pw_w, pw_b), pw_w.shape[0]))
        self._fold_key, self._fold = key, (fold, None if self.fold_out_conv else (ow, ob))
        return self._fold

    def conv_stack(self, d, variant=None):
        """out_conv(hidden_blocks(block1(d))), network.py:560-563, on csrc/conv_stack.hip: one fused
        kernel per block, two ping-pong maps."""
        if variant is None:
            if self.conv_precision not in ("fp32", "fp16", "amp", "bf16"):
                raise ValueError("conv_precision must be 'fp32', 'fp16' (1x1 operands), 'amp' (fp16 operands and maps) or 'bf16' "
                                 "(bf16 operands and maps)")
            if self.conv_precision == "bf16":
                # the same conditions as "amp" below; where they do not hold there is no fp32-map kernel with bf16 operands to fall
                # back on, and an fp16 kernel is not this class: the modules under torch's own bf16 autocast
                if d.shape[-1] % 4 == 0 and d.shape[-1] == d.shape[-2] and len(self.hidden_blocks) > 0:
                    return self._conv_stack_bf16(d, *self.folded_stack(bf16=True))
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    h = self.hidden_blocks(self.block1(d))
                return self.out_conv(h.float())
        fold, out_conv = self.folded_stack()
        if variant is None:
            # (a one-block stack has no map between blocks: fp32 in, fp32 out is the fp16-operand kernel's job -- ADVICE r2)
            if self.conv_precision == "amp" and d.shape[-1] % 4 == 0 and d.shape[-1] == d.shape[-2] and len(fold) > 1:
                return self._conv_stack_half(d, fold, out_conv)
            variant = 2 if self.conv_precision in ("fp16", "amp") else 0
        x, bufs = d, [None, None]
        for i, (packed, M) in enumerate(fold):
            if bufs[i & 1] is None or bufs[i & 1].shape[1] != M:
                bufs[i & 1] = torch.empty((d.shape[0], M) + tuple(d.shape[2:]), device=d.device, dtype=torch.float32)
            x = ops.conv_block(x, packed, M, out=bufs[i & 1], variant=variant)
        return x if out_conv is None else ops.pointwise_conv(x, out_conv[0], out_conv[1])

    def _conv_stack_half(self, d, fold, out_conv, block=ops.conv_block_half):
        """The reference's amp=True class (network.py:560-562: autocast around block1 + hidden_blocks): the maps between
        blocks are float16 in HBM (ops.conv_block_half); out_conv runs on float32 (`.float()`, :563) -- folded into the
        last block, which then writes float32."""
        x, C, bufs = d, d.shape[1], [None, None]
        for i, (packed, M) in enumerate(fold):
            last = i == len(fold) - 1
            x = block(x, packed, C, M, None if last else bufs[i & 1], not last)
            if not last:
                bufs[i & 1] = x
            C = M
        return x if out_conv is None else ops.pointwise_conv(x, out_conv[0], out_conv[1])

    def _conv_stack_bf16(self, d, fold, out_conv):
        """The same under amp_dtype=torch.bfloat16: bf16 maps between the blocks (ops.conv_block_bf16), fold packed by
        folded_stack(bf16=True); the first block reads the float32 d, the last one writes float32."""
        return self._conv_stack_half(d, fold, out_conv, block=ops.conv_block_bf16)

    def forward(self, num_grid, x, y, flow, scale_factor=1, logits=None, reuse_d=None):
        """reuse_d (not in the reference): a one-element list owned by the caller's loop over the iterations at one scale
        (network.py:257-268).  It holds the concat tensor of the previous iteration -- same x, same num_grid -- whose grid_feature
        planes are kept instead of regathered (results identical), and receives this call's.  The slot lives in the caller's
        frame, not on the module: two host threads driving one model cannot pick up each other's tensor; and it is only filled
        when the tensor cannot be part of an autograd graph (may_reuse_d)."""
        prev = reuse_d[0] if reuse_d is not None else None
        reusable = reuse_d is not None and self.may_reuse_d(x, y, flow)
        d, local_corr = self.assemble(num_grid, x, y, flow, scale_factor, reuse=prev if reusable else None)
        if reuse_d is not None:
            reuse_d[0] = d if reusable else None
        out = self.apply_stack(d)
        return out[:, :2], out[:, 2:3], local_corr

    def apply_stack(self, d):
        """out_conv(hidden_blocks(block1(d))), network.py:560-563, on whichever path this refiner's mode and settings select"""
        if self._hip_stack_supported():
            return self.conv_stack(d)
        if self._hip_train_stack_supported(d):
            # out_conv is not folded here: its parameters take their own gradients, and a 3-channel 1x1 needs no kernel
            return self.out_conv(self._train_stack_hip(d).float())
        if self._hip_amp_train_stack_supported(d):
            # fp16 maps between the nine blocks; the last y is fp16 and out_conv runs on fp32, as network.py:563 does
            return self.out_conv(self._train_stack_hip(d, amp=True).float())
        if self._hip_bf16_train_stack_supported(d):
            # the same with bf16 maps
            return self.out_conv(self._train_stack_hip(d, amp=torch.bfloat16).float())
        with torch.autocast("cuda", enabled=bool(self.amp), dtype=self.amp_dtype):
            h = self.hidden_blocks(self.block1(d))
        return self.out_conv(h.float())


def _refiner_for(feat_dim, disp_dim, radius):
    """The constructor arguments GFNet uses for each scale (model/network.py:79-154)."""
    has_corr = radius > 0
    dim = 2 * feat_dim + disp_dim + ((2 * radius + 1) ** 2 if has_corr else 0)
    return ConvRefiner(dim, dim, 2 + 1, kernel_size=5, dw=True, hidden_blocks=8, displacement_emb="linear",
                       displacement_emb_dim=disp_dim, local_corr_num=radius, corr_in_other=has_corr, amp=True,
                       disable_local_corr_grad=True, bn_momentum=0.01)


class GFNet(nn.Module):
    """Grid-based dense matcher, hot path on MI355X (reference: model/network.py:17-440)."""

    def __init__(self, conf, sample_mode="threshold_balanced", exact_softmax=False, amp=True, amp_dtype=torch.float16,
                 initial_res=(448, 448), upsample_res=(560, 560), symmetric=False, upsample_preds=False,
                 attenuate_cert=False, backbone=None, conv_refiner=None):
        super().__init__()
        m = conf["matcher"]
        self.num_grid = list(m["num_grid"])
        self.radius = list(m["radius"])
        self.num_itr = list(m["num_itr"])
        self.backbone_state, self.ignored_backbone_keys = {}, []
        if backbone is None and os.environ.get("GFNET_COMPAT_BACKBONE", "") == "reference":
            # the reference's own constructor call (test.py:25-30) has no backbone argument: with this switch the DINOv2 + decoder + FPN
            # of the user's checkout are assembled here, as the reference's constructor does (network.py:44-65)
            from ..reference_backbone import reference_backbone

            # GFNET_COMPAT_DECODER=hip: the native cross-view decoder (model/crossview_decoder.py) in place of the checkout's, whose
            # shipped attention type needs flash_attn (hip_fused: the same with its blocks fused around the attention in fp16 eval());
            # unset: the checkout's class, as before
            # GFNET_COMPAT_DECODER_TRAIN=hip: the native decoder trains its blocks through the backward kernels of
            # csrc/decoder_block.hip (train_block_impl="hip"); unset: torch autograd, as before
            # GFNET_COMPAT_FPN=hip: the native FPN encoder, merge layer and decoder (model/fpn.py) in place of the checkout's
            # `model.FPN`, one fused launch per layer in eval(); unset: the checkout's classes, as before
            # GFNET_COMPAT_FPN_PRECISION=fp16 (with GFNET_COMPAT_FPN=hip): the native FPN in its fp16 class, fp16 pyramids handed to
            # the matcher as stored; unset: fp32, as before
            # GFNET_COMPAT_DINO=hip: the native DINOv2 ViT (model/dinov2.py) in place of the checkout's `model.transformer`, attention
            # and block seams in HIP in fp16 eval(); unset: the checkout's class, as before
            backbone = reference_backbone(conf, amp=amp, amp_dtype=amp_dtype, decoder=os.environ.get("GFNET_COMPAT_DECODER") or "checkout",
                                          fpn=os.environ.get("GFNET_COMPAT_FPN") or "checkout",
                                          dino=os.environ.get("GFNET_COMPAT_DINO") or "checkout",
                                          fpn_precision=os.environ.get("GFNET_COMPAT_FPN_PRECISION") or "fp32",
                                          decoder_train_impl=os.environ.get("GFNET_COMPAT_DECODER_TRAIN") or "torch")
        self.backbone = backbone
        if conv_refiner is None:
            chs = conf["encoder_cfg"]["feat_chs"]  # coarse to fine: [64, 32, 16, 8]
            feat = [chs[0], chs[0], chs[1], chs[2], chs[3]]
            conv_refiner = nn.ModuleDict({s: _refiner_for(feat[i], m["displacement_dim"][i], self.radius[i])
                                          for i, s in enumerate(SCALES)})
        self.conv_refiner = conv_refiner
        self.sample_mode = sample_mode
        self.sample_thresh = 0.05
        self.upsample_preds = upsample_preds
        self.upsample_res = upsample_res
        self.symmetric = symmetric
        self.attenuate_cert = attenuate_cert
        self.h_resized, self.w_resized = initial_res
        self.initial_res = initial_res
        self.exact_softmax = exact_softmax
        self.amp, self.amp_dtype = amp, amp_dtype
        self.ransac_iters = 2000  # OpenCV's default maxIters for findHomography

    # ---- checkpoints ---------------------------------------------------------------------------------
    REFERENCE_BACKBONE_PREFIXES = ("dino_decoder", "encoder", "decoder", "merge_layer")  # the reference's registered submodules
                                                                                         # beside conv_refiner (network.py:47-60)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Accepts a FULL reference checkpoint (test.py:37-38: `model.load_state_dict(states["model"])`): `conv_refiner.*` entries load
        as they are (same parameter names); an entry of the reference's backbone goes to `backbone.<name>` when the attached backbone
        is a module that has it.  Without such a module the entries are NOT dropped: they are kept (`self.backbone_state`, names in
        `self.ignored_backbone_keys`), a warning says how many, and they are loaded the moment a backbone module is assigned to
        `model.backbone` (construct -> load_state_dict -> assign the backbone must not leave it at its random init).
        Anything else is reported by torch as usual."""
        own = self.state_dict()
        routed, pending = {}, {}
        for k, v in state_dict.items():
            if k in own:
                routed[k] = v
            elif "backbone." + k in own:
                routed["backbone." + k] = v
            elif k.split(".")[0] in self.REFERENCE_BACKBONE_PREFIXES:
                pending[k] = v
            else:
                routed[k] = v
        self.backbone_state = pending
        self.ignored_backbone_keys = list(pending)
        if pending:
            import warnings

            prefixes = sorted({k.split(".")[0] for k in pending})
            warnings.warn(f"GFNet.load_state_dict: {len(pending)} backbone entries ({', '.join(prefixes)}.*) have no module to go to yet; "
                          "they are kept in model.backbone_state and are loaded when an nn.Module backbone with those submodules is "
                          "assigned to model.backbone (a plain callable backbone has to load its own weights)", stacklevel=2)
        return super().load_state_dict(routed, strict=strict, assign=assign)

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if name == "backbone" and isinstance(value, nn.Module) and getattr(self, "backbone_state", None):
            # the checkpoint came first (test.py's order with a backbone attached afterwards): hand the kept entries over now
            have = value.state_dict()
            take = {k: v for k, v in self.backbone_state.items() if k in have}
            if take:
                value.load_state_dict(take, strict=False)
            self.backbone_state = {k: v for k, v in self.backbone_state.items() if k not in take}
            self.ignored_backbone_keys = list(self.backbone_state)

    # ---- the two methods GFNet.forward calls at scale 16 (network.py:251-252) -------------------
    def corr_volume(self, feat0, feat1):
        return ops.corr_volume(feat0, feat1)

    def pos_embed(self, corr_volume):
        return ops.pos_embed(corr_volume)

    # ---- backbone hook ---------------------------------------------------------------------------
    def extract_features(self, x, upsample=False):
        if self.backbone is None:
            raise NotImplementedError(
                "no backbone attached: the DINOv2/FPN feature extractor stays ordinary PyTorch-ROCm host code and is not "
                "part of gfnet_amd; pass backbone=... or call forward_pyramids()/match_pyramids() with feature pyramids")
        return self.backbone(x, upsample)

    def upsample_grids(self, hs):
        """num_grid_up of match() (network.py:329) and the matching radii / iteration counts."""
        g = int(hs / 14)
        grids = [g, 2 * g, 4 * g, 8 * g]
        return grids, self.radius[-len(grids):], self.num_itr[-len(grids):]

    # ---- coarse-to-fine loop (network.py:230-281) ---------------------------------------------------
    def forward_pyramids(self, features0, features1, image_hw, symmetric=False, upsample=False, scale_factor=1,
                         pre_corresps=None):
        """GFNet.forward after feature extraction.  features*: dict scale -> (B,c,h,w), coarse to
        fine, keys "16".."1" (or "8".."1" when upsample).  image_hw: (H0, W0) of the network input."""
        H0, W0 = image_hw
        # symmetric (network.py:213-222): the reference concatenates (A,B) and (B,A) pyramids; here the
        # kernels index the two directions virtually, nothing is copied
        if upsample:
            num_grid, _, num_itr = self.num_grid_up, self.radius_up, self.num_itr_up
        else:
            num_grid, num_itr = self.num_grid, self.num_itr
        scales = list(features0.keys())
        corresps = {}
        flow = certainty = None
        for idx, scale in enumerate(scales):
            f0, f1 = features0[scale], features1[scale]
            if idx == 0:
                if upsample:
                    if pre_corresps is None:
                        raise ValueError("upsampling refinement needs pre_corresps")
                    flow, certainty = ops.interpolate_bilinear_pair(pre_corresps["flow"], pre_corresps["certainty"], num_grid[0])  # :238-249
                else:
                    flow = ops.corr_softargmax(f0, f1, symmetric=symmetric)                      # :251-252
                    certainty = torch.zeros((flow.shape[0], 1) + tuple(flow.shape[2:]), device=flow.device)  # :253
            corresps[scale] = {}
            fuse_resize = (ops.FUSE_UPDATE_RESIZE and not torch.is_grad_enabled() and scale != "1" and num_itr[idx] >= 1
                           and num_grid[idx + 1] in (flow.shape[-1], 2 * flow.shape[-1]))
            disp_prev = torch.empty_like(flow) if num_itr[idx] > 1 else None  # carried between the iterations of one scale
            for itr in range(num_itr[idx]):
                ref = self.conv_refiner[scale]
                # later iterations at a scale see the same features and grid: the refiner keeps the grid_feature planes of
                # its previous concat tensor (ConvRefiner.forward, reuse_d) instead of regathering them.  The slot is a local
                # of this loop (never module state) and dies with the scale.
                if itr == 0:
                    d_slot = [None] if (num_itr[idx] > 1 and getattr(ref, "supports_reuse_d", False)) else None
                if d_slot is not None:
                    d_flow, d_cert, _ = ref(num_grid[idx], f0, f1, flow, scale_factor=scale_factor, reuse_d=d_slot)
                else:
                    d_flow, d_cert, _ = ref(num_grid[idx], f0, f1, flow, scale_factor=scale_factor)
                # each iteration's result is kept (corresps): out-of-place update straight from the refiner's outputs
                if itr == num_itr[idx] - 1 and fuse_resize:  # the scale's last update and the resize below in one launch
                    flow, certainty, flow_next, cert_next = ops.flow_update_resize(
                        flow, certainty, d_flow, d_cert, disp_prev, int(scale), W0, H0, num_grid[idx + 1],
                        zero_small=not self.training, first_iteration=(itr == 0))                 # :262-268 + :271-281
                else:
                    flow, certainty = ops.flow_update(flow, certainty, d_flow, d_cert, disp_prev, int(scale), W0, H0,
                                                      zero_small=not self.training, first_iteration=(itr == 0))  # :262-268
                corresps[scale][itr + 1] = {"flow": flow, "certainty": certainty}
            if fuse_resize:
                flow, certainty = flow_next, cert_next
            elif scale != "1":                                                                    # :271-281
                flow, certainty = ops.interpolate_bilinear_pair(flow, certainty, num_grid[idx + 1])
        return corresps

    def forward(self, batch, symmetric=False, upsample=False, scale_factor=1, pre_corresps=None, visualization=False):
        im0, im1 = batch["im_A"], batch["im_B"]
        H0, W0 = im0.shape[-2:]
        f0, f1 = self.extract_features(torch.cat([im0, im1], dim=0), upsample)
        return self.forward_pyramids(f0, f1, (H0, W0), symmetric=symmetric, upsample=upsample, scale_factor=scale_factor,
                                     pre_corresps=pre_corresps)

    # ---- match (network.py:285-384) ------------------------------------------------------------------
    def _finish_match(self, corresps, corresps_up, batched):
        num_itr = self.num_itr_up if corresps_up is not None else self.num_itr
        last = (corresps_up if corresps_up is not None else corresps)["1"][num_itr[-1]]
        c16 = corresps["16"][self.num_itr[0]]["certainty"] if self.attenuate_cert else None
        warp, certainty = ops.match_post(last["flow"], last["certainty"], c16, symmetric=self.symmetric)
        return (warp, certainty) if batched else (warp[0], certainty[0])

    @torch.inference_mode()
    def match_pyramids(self, pyr0, pyr1, pyr0_up=None, pyr1_up=None, batched=True):
        """match() on precomputed feature pyramids: the 448 pass, the optional 560 refinement pass
        seeded by it (upsample_preds), certainty attenuation, post-processing."""
        return self.match_second_pass(self.match_first_pass(pyr0, pyr1), pyr0_up, pyr1_up, batched=batched)

    # The two halves of match_pyramids as calls of their own: a host that streams batches can run the first pass of batch k + 1
    # beside the refinement pass of batch k (each on a HIP stream of its own; every kernel still sees the whole batch).
    @torch.inference_mode()
    def match_first_pass(self, pyr0, pyr1):
        """The first (initial-resolution) coarse-to-fine pass: network.py:285-331.  Returns its corresps."""
        if self.training:  # (train() walks every submodule: 50 attribute writes per call on a host-bound path)
            self.train(False)
        return self.forward_pyramids(pyr0, pyr1, (self.h_resized, self.w_resized), symmetric=self.symmetric)

    @torch.inference_mode()
    def match_second_pass(self, corresps, pyr0_up=None, pyr1_up=None, batched=True):
        """The optional refinement pass seeded by the first pass's corresps (upsample_preds), certainty attenuation,
        post-processing: network.py:332-384."""
        corresps_up = None
        if self.upsample_preds:
            hs, ws = self.upsample_res
            up = self.upsample_grids(hs)
            if getattr(self, "_up_key", None) != (hs, tuple(self.radius), tuple(self.num_itr)):  # nn.Module.__setattr__ is not free: set once
                self.num_grid_up, self.radius_up, self.num_itr_up = up
                self._up_key = (hs, tuple(self.radius), tuple(self.num_itr))
            if pyr0_up is None:
                raise ValueError("upsample_preds=True needs the feature pyramids of the upsample resolution")
            sf = math.sqrt(hs * ws / (self.w_resized * self.h_resized))
            corresps_up = self.forward_pyramids(pyr0_up, pyr1_up, (hs, ws), symmetric=self.symmetric, upsample=True,
                                                scale_factor=sf, pre_corresps=corresps["1"][self.num_itr[-1]])
        return self._finish_match(corresps, corresps_up, batched)

    @torch.inference_mode()
    def match(self, im0, im1, *args, batched=True):
        """Same contract as the reference: paths / PIL images / tensors in, (warp, certainty) out.
        Needs a backbone; image resize + ImageNet normalisation run in one HIP kernel with the
        reference's interpolation modes (network.py:293-346: bilinear for path inputs and for the upsample pass,
        bicubic for PIL / tensor inputs, no antialiasing)."""
        from ..utils.image import load_pair, resize_normalise

        im_a, im_b, batched, mode = load_pair(im0, im1, batched)
        im_a, im_b = im_a.cuda(), im_b.cuda()

        def pyramids(res, upsample):
            m = "bilinear" if upsample else mode
            return self.extract_features(torch.cat([resize_normalise(im_a, res, m), resize_normalise(im_b, res, m)]), upsample)

        p0, p1 = pyramids((self.h_resized, self.w_resized), False)
        u0 = u1 = None
        if self.upsample_preds:
            u0, u1 = pyramids(self.upsample_res, True)
        return self.match_pyramids(p0, p1, u0, u1, batched=batched)

    @torch.inference_mode()
    def match_batch(self, im_a, im_b, mode="bicubic"):
        """match() for B pairs at once: im_a, im_b (B,3+,H,W) float tensors in [0,1] (what ToTensor gives for the PIL
        images test.py passes, hence the bicubic first pass; the upsample pass is bilinear as in network.py:342-344).
        Returns warp (B,G,2G,4) and certainty (B,G,2G)."""
        from ..utils.image import resize_normalise

        im_a, im_b = im_a.cuda(), im_b.cuda()

        def pyramids(res, upsample):
            m = "bilinear" if upsample else mode
            return self.extract_features(torch.cat([resize_normalise(im_a, res, m), resize_normalise(im_b, res, m)]), upsample)

        p0, p1 = pyramids((self.h_resized, self.w_resized), False)
        u0 = u1 = None
        if self.upsample_preds:
            u0, u1 = pyramids(self.upsample_res, True)
        return self.match_pyramids(p0, p1, u0, u1, batched=True)

    # match_batch in two calls, for a host that streams batches through three HIP streams (gfnet_amd.evaluate): the first pass of
    # batch k + 1 runs beside the refinement pass of batch k.  match_batch_second(match_batch_first(a, b)) == match_batch(a, b).
    @torch.inference_mode()
    def match_batch_first(self, im_a, im_b, mode="bicubic"):
        from ..utils.image import resize_normalise

        im_a, im_b = im_a.cuda(), im_b.cuda()
        res = (self.h_resized, self.w_resized)
        p0, p1 = self.extract_features(torch.cat([resize_normalise(im_a, res, mode), resize_normalise(im_b, res, mode)]), False)
        return {"corresps": self.match_first_pass(p0, p1), "im_a": im_a, "im_b": im_b}

    @torch.inference_mode()
    def match_batch_second(self, state):
        from ..utils.image import resize_normalise

        u0 = u1 = None
        if self.upsample_preds:
            ims = torch.cat([resize_normalise(state["im_a"], self.upsample_res, "bilinear"),
                             resize_normalise(state["im_b"], self.upsample_res, "bilinear")])
            u0, u1 = self.extract_features(ims, True)
        return self.match_second_pass(state["corresps"], u0, u1, batched=True)

    # ---- sample (network.py:385-414) --------------------------------------------------------------------
    def sample(self, matches, certainty, num=5_000):
        matches = matches.reshape(-1, 4)
        certainty = certainty.reshape(-1)
        if "threshold" in self.sample_mode:
            certainty = ops.threshold_certainty(certainty, self.sample_thresh)
        expansion = 4 if "balanced" in self.sample_mode else 1
        good = torch.multinomial(certainty, num_samples=min(expansion * num, len(certainty)), replacement=False)
        good_matches, good_certainty = matches[good], certainty[good]
        if "balanced" not in self.sample_mode:
            return good_matches, good_certainty
        # the reference uses half precision and the full set on a GPU (network.py:406-407)
        density = kde(good_matches, std=0.1, half=True, down=1)
        p = ops.balance_weights(density.float())
        balanced = torch.multinomial(p, num_samples=min(num, len(good_certainty)), replacement=False)
        return good_matches[balanced], good_certainty[balanced]


def sample_batched(model, warp, certainty, num=5_000, sampler="hip"):
    """GFNet.sample for a batch of pairs in one go: warp (B,G,Gw,4), certainty (B,G,Gw) ->
    matches (B,num,4), certainty (B,num).  Same steps as model/network.py:385-414 per pair (the
    reference evaluates pairs one at a time); the densities come from one batched KDE launch and the two draws without
    replacement from ops.sample_without_replacement (sampler="hip": the exponential race torch.multinomial runs, seeded
    from torch's CPU generator) or from torch.multinomial itself (sampler="torch")."""
    B = warp.shape[0]
    m = warp.reshape(B, -1, 4)
    c = certainty.reshape(B, -1)
    expansion = 4 if "balanced" in model.sample_mode else 1
    n1 = min(expansion * num, c.shape[1])
    thr = model.sample_thresh if "threshold" in model.sample_mode else None
    if sampler == "hip":
        # the certainty threshold (network.py:391-393) is applied on the fly by the draw and by the gather
        good = ops.sample_without_replacement(c, n1, one_above=thr)                  # (B,n1)
        gm, gc = ops.gather_matches(m, c, good, one_above=thr)
    else:
        if thr is not None:
            c = ops.threshold_certainty(c, thr)
        good = torch.multinomial(c, num_samples=n1, replacement=False)
        gm = torch.gather(m, 1, good[..., None].expand(B, n1, 4)).contiguous()
        gc = torch.gather(c, 1, good)
    if "balanced" not in model.sample_mode:
        return gm, gc
    density = ops.kde_density(gm, std=0.1, round_fp16=True)                          # half inputs, fp32 sums
    p = ops.balance_weights(density, round_fp16=True)
    n2 = min(num, n1)
    if sampler == "hip":
        return ops.gather_matches(gm, gc, ops.sample_without_replacement(p, n2))
    bal = torch.multinomial(p, num_samples=n2, replacement=False)
    return torch.gather(gm, 1, bal[..., None].expand(B, n2, 4)).contiguous(), torch.gather(gc, 1, bal)


