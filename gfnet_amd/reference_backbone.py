"""The reference's feature extractor, built from the USER'S OWN GFNet checkout, as a `backbone=` for gfnet_amd's GFNet.

BASELINE north_star: "host code stays PyTorch-ROCm for the FPN/transformer backbone".  By default nothing of that backbone is taken
from this package (decoder="hip", fpn="hip" and dino="hip" opt into its own cross-view decoder, FPN and DINOv2 ViT,
model/crossview_decoder.py, model/fpn.py and model/dinov2.py; with all three nothing of a checkout is imported); this module
only *assembles* it from the checkout's classes when one is importable (`model.FPN`,
`model.crossview_decoder_light`, `model.transformer` -- with compat/ on sys.path those still resolve to the checkout, see
compat/model/__init__.py) and states the data flow of `GFNet.extract_features` (reference model/network.py:156-201) around them:

    DINOv2 ViT-L/14 patch tokens (frozen, amp dtype)  -> cross-view decoder -> stride-16 features (B, 64, H/14, W/14)
    FPN encoder on the images -> conv31 += merge_layer(cat(conv31, resized ViT features)) -> FPN decoder -> strides 8, 4, 2, 1
    pyramids = {"16": vit, "8": feat1, "4": feat2, "2": feat3, "1": feat4}, first half of the batch = image A, second = image B;
    the refinement pass (upsample=True) drops "16".

The submodule names are the reference's (`dino_decoder`, `encoder`, `decoder`, `merge_layer`: network.py:57-65), so the entries of a
full reference checkpoint route into them (GFNet.load_state_dict); the ViT hangs in a plain list like the reference's `self.dino`
(network.py:56: kept out of the state dict, moved to the device lazily).
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

DINOV2_URL = "https://dl.fbaipublicfiles.com/dinov2/dinov2_vitl14/dinov2_vitl14_pretrain.pth"  # network.py:46


DECODERS = ("checkout", "hip", "hip_fused")
FPNS = ("checkout", "hip")
DINOS = ("checkout", "hip")


def _needed(decoder, fpn):
    return (("model.FPN",) if fpn == "checkout" else ()) + (("model.crossview_decoder_light",) if decoder == "checkout" else ())


def _check_choices(decoder, fpn, dino="checkout"):
    if decoder not in DECODERS:
        raise ValueError(f"decoder must be one of {DECODERS}, got {decoder!r}")
    if fpn not in FPNS:
        raise ValueError(f"fpn must be one of {FPNS}, got {fpn!r}")
    if dino not in DINOS:
        raise ValueError(f"dino must be one of {DINOS}, got {dino!r}")


def _check_fpn_train_impl(fpn, fpn_train_impl):
    if fpn_train_impl not in ("torch", "hip", "hip_fused"):
        raise ValueError(f"fpn_train_impl must be 'torch', 'hip' or 'hip_fused', got {fpn_train_impl!r}")
    if fpn_train_impl != "torch" and fpn != "hip":
        raise ValueError(f"fpn_train_impl={fpn_train_impl!r} needs fpn='hip': the checkout's FPN modules train through torch only")


def _check_fpn_precision(fpn, fpn_precision):
    if fpn_precision not in ("fp32", "fp16", "tf32"):
        raise ValueError(f"fpn_precision must be 'fp32', 'fp16' or 'tf32', got {fpn_precision!r}")
    if fpn_precision != "fp32" and fpn != "hip":
        raise ValueError(f"fpn_precision={fpn_precision!r} needs fpn='hip': the checkout's FPN modules run in fp32 only")


def _check_decoder_train_impl(decoder, decoder_train_impl):
    if decoder_train_impl not in ("torch", "hip"):
        raise ValueError(f"decoder_train_impl must be 'torch' or 'hip', got {decoder_train_impl!r}")
    if decoder_train_impl != "torch" and decoder == "checkout":
        raise ValueError(f"decoder_train_impl={decoder_train_impl!r} needs decoder='hip' or 'hip_fused': the checkout's decoder trains "
                         "through torch only")


def checkout_available(decoder="checkout", fpn="checkout"):
    """True when the reference's backbone modules that this choice takes from the checkout can be found on sys.path (nothing is
    imported).  decoder="hip" does without `model.crossview_decoder_light`, fpn="hip" without `model.FPN`: those are then this
    package's; with both, nothing is needed (the ViT apart, which is built only where none is passed in, and
    with dino="hip" is this package's too)."""
    import importlib.util

    needed = _needed(decoder, fpn)
    try:
        return all(importlib.util.find_spec(m) is not None for m in needed)
    except (ImportError, ValueError):
        return False


def _build_vit(dino_weights):
    from model.transformer import vit_large  # the checkout's DINOv2 (needs its own third-party imports, e.g. romatch)

    vit = vit_large(img_size=518, patch_size=14, init_values=1.0, ffn_layer="mlp", block_chunks=0).eval()  # network.py:48-54
    return _load_dino_weights(vit, dino_weights)


def _build_native_vit(dino_weights):
    from .model.dinov2 import vit_large  # this package's DINOv2 under the same parameter names: nothing of a checkout

    vit = vit_large(img_size=518, patch_size=14, init_values=1.0, ffn_layer="mlp", block_chunks=0).eval()
    return _load_dino_weights(vit, dino_weights)


def _load_dino_weights(vit, dino_weights):
    if dino_weights is None:
        dino_weights = os.environ.get("GFNET_DINOV2_WEIGHTS")
    if dino_weights is None:
        state = torch.hub.load_state_dict_from_url(DINOV2_URL, map_location="cpu")  # what the reference's constructor does
    elif isinstance(dino_weights, (str, os.PathLike)):
        state = torch.load(dino_weights, map_location="cpu")
    else:
        state = dino_weights
    vit.load_state_dict(state)
    return vit


def _resize_side(vit_feat, size):
    """The ViT map on the stride-8 grid (32 -> 56 at 448).  torch's GPU backward of F.interpolate scatters with atomics and raises
    under torch.use_deterministic_algorithms(True); a GPU map that needs a gradient under that flag goes through ops.resize_bilinear
    (the same resize, its backward a gather).  Every other call is F.interpolate."""
    if vit_feat.is_cuda and vit_feat.requires_grad and torch.is_grad_enabled() and torch.are_deterministic_algorithms_enabled():
        from . import ops

        return ops.resize_bilinear(vit_feat, size)
    return F.interpolate(vit_feat, size=size, mode="bilinear", align_corners=False)


class ReferenceBackbone(nn.Module):
    """`backbone(images, upsample) -> (pyramid_A, pyramid_B)` from the checkout's DINOv2 + CrossVITDecoder_noself + FPN.

    vit: an already built ViT (anything with `forward_features(x)["x_norm_patchtokens"]`); None builds the checkout's `vit_large`
    and loads `dino_weights` (a path, a state dict, $GFNET_DINOV2_WEIGHTS, or the reference's download URL in that order).

    decoder: "checkout" (default) builds the checkout's CrossVITDecoder_noself, which with the shipped attention_type "FLASH2" raises
    on its first forward where flash_attn is missing; "hip" builds gfnet_amd.model.crossview_decoder.CrossViewDecoder, the same
    module under the same parameter names with its attention core in HIP, and does not import the checkout's decoder;
    "hip_fused" builds the same module with block_impl="hip": in inference under fp16 or bf16 autocast (amp_dtype) each block is three HIP launches
    (csrc/decoder_block.hip around the attention), every other call is "hip" exactly.

    fpn: "checkout" (default) builds the checkout's FPNEncoder, FPNDecoder_concat and merge layer; "hip" builds
    gfnet_amd.model.fpn's, the same modules under the same parameter names with one fused HIP launch per layer in eval(), and does
    not import `model.FPN`.

    dino: which ViT is built where none is passed in.  "checkout" (default) builds the checkout's `vit_large`, which imports
    `model.transformer` and with it the checkout's third-party imports; "hip" builds gfnet_amd.model.dinov2.vit_large, the same model
    under the same parameter names (`dino_weights` load strictly, exactly as above) with its attention and the seams of its blocks
    in HIP in eval() in either 16-bit class: the ViT is cast to amp_dtype, and fp16 and bf16 both run its kernels.  With decoder="hip", fpn="hip" and dino="hip" nothing of a checkout is imported.

    fpn_train_impl: "torch" (default), "hip" or "hip_fused" ("hip" with the decoder's 2x upsample inside the innerN op), the
    train_conv_impl of the three native FPN modules: what they run under train() (see gfnet_amd/model/fpn.py).  The checkout's modules have no such switch: anything but "torch" with fpn="checkout" raises ValueError.

    fpn_precision: "fp32" (default) or "fp16", the conv_precision of the three native FPN modules (see gfnet_amd/model/fpn.py): with
    "fp16" their eval() HIP path keeps fp16 maps and runs on the matrix core, and in eval() on the GPU ALL FIVE LEVELS ARE RETURNED IN
    fp16 as stored (the stride-16 map is cast to fp16 too), not widened: GFNet.match / match_batch read fp16 pyramids directly.
    train() and CPU tensors return fp32 levels as before.  "tf32" is the reference's own TF32 class of the FPN's convolutions, for the
    eval() and the train() HIP paths (fpn_train_impl "hip" / "hip_fused"): split-bf16 operands on the matrix core, fp32 maps, the five
    levels returned in fp32 as under "fp32".  Either needs fpn="hip", else ValueError.

    decoder_train_impl: "torch" (default) or "hip", the train_block_impl of the native cross-view decoder: "hip" trains its blocks
    through the backward kernels of csrc/decoder_block.hip under fp16 or bf16 autocast: amp_dtype=torch.bfloat16 selects the bf16 class of
    the attention and of the blocks, with nothing else to set (see gfnet_amd/model/crossview_decoder.py).  Anything
    but "torch" with decoder="checkout" raises ValueError."""

    def __init__(self, conf, amp=True, amp_dtype=torch.float16, vit=None, dino_weights=None, decoder="checkout", fpn="checkout",
                 dino="checkout", fpn_train_impl="torch", decoder_train_impl="torch", fpn_precision="fp32"):
        super().__init__()
        _check_choices(decoder, fpn, dino)
        _check_fpn_train_impl(fpn, fpn_train_impl)
        _check_fpn_precision(fpn, fpn_precision)
        self.fpn_precision = fpn_precision
        _check_decoder_train_impl(decoder, decoder_train_impl)
        self.fpn = fpn
        if fpn == "hip":
            from .model.fpn import FPNDecoder_concat, FPNEncoder, merge_layer
        else:
            from model.FPN import FPNDecoder_concat, FPNEncoder, Swish

        self.amp, self.amp_dtype = amp, amp_dtype
        if vit is None:
            vit = _build_native_vit(dino_weights) if dino == "hip" else _build_vit(dino_weights)
        for p in vit.parameters():
            p.requires_grad = False
        self.dino = [vit]
        chs = list(conf["encoder_cfg"]["feat_chs"])  # coarse to fine
        if decoder in ("hip", "hip_fused"):
            from .model.crossview_decoder import CrossViewDecoder

            self.dino_decoder = CrossViewDecoder(conf, block_impl="hip" if decoder == "hip_fused" else "torch",
                                                 train_block_impl=decoder_train_impl)
        else:
            from model.crossview_decoder_light import CrossVITDecoder_noself

            self.dino_decoder = CrossVITDecoder_noself(conf=conf, upsample=False)
        native = {"train_conv_impl": fpn_train_impl, "conv_precision": fpn_precision} if fpn == "hip" else {}
        self.encoder = FPNEncoder(feat_chs=chs[::-1], **native)
        self.decoder = FPNDecoder_concat(feat_chs=chs[::-1], **native)
        if fpn == "hip":
            self.merge_layer = merge_layer(chs[0], **native)
        else:
            self.merge_layer = nn.Sequential(nn.Conv2d(2 * chs[0], chs[0], kernel_size=3, padding=1), nn.BatchNorm2d(chs[0]), Swish())

    def _vit_tokens(self, x):
        vit = self.dino[0]
        p = next(vit.parameters(), None)
        if p is not None and (p.device != x.device or (x.is_cuda and p.dtype != self.amp_dtype)):
            vit = self.dino[0] = vit.to(x.device).to(self.amp_dtype if x.is_cuda else p.dtype)
            p = next(vit.parameters())
        with torch.no_grad():
            return vit.forward_features(x.to(p.dtype) if p is not None else x)["x_norm_patchtokens"]

    def forward(self, x, upsample=False):
        n2, ch, H, W = x.shape
        hv, wv = H // 14 * 14, W // 14 * 14
        tokens = self._vit_tokens(x if (H, W) == (hv, wv) else F.interpolate(x, (hv, wv), mode="bilinear", align_corners=False))
        ta, tb = tokens.chunk(2)
        with torch.autocast(device_type="cuda", enabled=bool(self.amp) and x.is_cuda, dtype=self.amp_dtype):
            va, vb = self.dino_decoder(ta, tb, vit_shape=(n2 // 2, ch, hv // 14, wv // 14))
        vit_feat = torch.cat((va.float(), vb.float()))
        c0, c1, c2, c3 = self.encoder(x)
        side = vit_feat if tuple(vit_feat.shape[2:]) == (H // 8, W // 8) else _resize_side(vit_feat, (H // 8, W // 8))
        # (the native merge layer takes both maps and adds conv31 itself: one launch, no concatenation)
        c3 = self.merge_layer(c3, side) if self.fpn == "hip" else c3 + self.merge_layer(torch.cat((c3, side), dim=1))
        levels = [vit_feat] + list(self.decoder(c0, c1, c2, c3))
        # the fp16 class hands its maps on as stored (fp16 where its HIP path ran: eval() on the GPU), every level in that one dtype
        keep = levels[-1].dtype if self.fpn_precision == "fp16" and levels[-1].dtype == torch.float16 else torch.float32
        pyr_a, pyr_b = {}, {}
        for name, t in zip(("16", "8", "4", "2", "1"), levels):
            if upsample and name == "16":
                continue
            a, b = t.to(keep).chunk(2)
            pyr_a[name], pyr_b[name] = a.contiguous(), b.contiguous()
        return pyr_a, pyr_b


def reference_backbone(conf, amp=True, amp_dtype=torch.float16, vit=None, dino_weights=None, decoder="checkout", fpn="checkout",
                       dino="checkout", fpn_train_impl="torch", decoder_train_impl="torch", fpn_precision="fp32"):
    """Build the backbone from the checkout on sys.path; raises ImportError with the reason when a module this choice needs from it
    is missing.  decoder, fpn, dino, fpn_train_impl, decoder_train_impl, fpn_precision: see ReferenceBackbone."""
    _check_choices(decoder, fpn, dino)
    _check_fpn_train_impl(fpn, fpn_train_impl)
    _check_fpn_precision(fpn, fpn_precision)
    _check_decoder_train_impl(decoder, decoder_train_impl)
    if not checkout_available(decoder, fpn):
        raise ImportError(f"no KN-Zhang/GFNet checkout on sys.path: {' / '.join(f'`{m}`' for m in _needed(decoder, fpn))} cannot be found "
                          "(put the checkout behind compat/ on PYTHONPATH, or run the script through compat/run.py)")
    return ReferenceBackbone(conf, amp=amp, amp_dtype=amp_dtype, vit=vit, dino_weights=dino_weights, decoder=decoder, fpn=fpn,
                             dino=dino, fpn_train_impl=fpn_train_impl, decoder_train_impl=decoder_train_impl, fpn_precision=fpn_precision)
