"""The frozen DINOv2 ViT of the feature extractor, with its attention core and the seams of its blocks in HIP.

A mirror, in this package's words, of the reference's `DinoVisionTransformer` and `vit_large` (model/transformer/dinov2.py:43-155,
333-343) and of the layers it builds them from (layers/patch_embed.py, attention.py:51-110, block.py:36-107, mlp.py, layer_scale.py),
for the configuration GFNet builds (model/network.py:48-54): ffn_layer "mlp", block_chunks 0, no drop path.  Parameter names are the
reference's, so the official `dinov2_vitl14_pretrain.pth` loads with strict=True:

    cls_token  pos_embed  mask_token  patch_embed.proj.{weight,bias}  norm.{weight,bias}
    blocks.{i}.  norm1.*  attn.qkv.*  attn.proj.*  ls1.gamma  norm2.*  mlp.fc1.*  mlp.fc2.*  ls2.gamma

Every parameter is frozen, as the reference's constructor leaves them (dinov2.py:154-155).  Two paths over the same parameters:

  * impl "hip" (the default), taken in eval() on CUDA in fp16 or bf16 at head dim 64 without masks: attention is ONE
    ops.self_attention (fp16) or ops.self_attention_bf16 launch on the packed qkv projection (csrc/self_attn.hip: no permutes, no
    copies), and each of a block's two seams -- LayerScale multiply, residual add, the LayerNorm that follows -- ONE ops.ls_add_layernorm launch
    (csrc/layernorm.hip); the last block's second seam carries the model's final `norm`.  Linear layers, the patch convolution and
    GELU are torch ops.  No autograd on this path.
  * everything else -- the CPU, fp32, `masks` given, train(), impl "torch" -- runs torch ops as the reference writes
    them (F.scaled_dot_product_attention on the permuted projection).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

IMPLS = ("hip", "torch")
HIP_HEAD_DIM = 64
HIP_DTYPES = (torch.float16, torch.bfloat16)  # the two 16-bit classes the kernels are instantiated for


def _check_impl(impl):
    if impl not in IMPLS:
        raise ValueError(f"impl must be one of {IMPLS}, got {impl!r}")
    return impl


class PatchEmbed(nn.Module):
    """layers/patch_embed.py:26-82: (B, C, H, W) -> (B, H/p * W/p, D)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        hw = img_size if isinstance(img_size, tuple) else (img_size, img_size)
        p = patch_size if isinstance(patch_size, tuple) else (patch_size, patch_size)
        self.img_size, self.patch_size = hw, p
        self.patches_resolution = (hw[0] // p[0], hw[1] // p[1])
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=p, stride=p)

    def forward(self, x):
        H, W = x.shape[2:]
        if H % self.patch_size[0] or W % self.patch_size[1]:
            raise ValueError(f"PatchEmbed: image height and width must be multiples of the patch size {self.patch_size}, got {(H, W)}")
        return self.proj(x).flatten(2).transpose(1, 2)


class Attention(nn.Module):
    """layers/attention.py:51-101 (what MemEffAttention falls back to without xformers, :106-110)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, proj_bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)

    def forward(self, x, hip=False):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads)
        if hip:
            attn = ops.self_attention_bf16 if qkv.dtype == torch.bfloat16 else ops.self_attention
            return self.proj(attn(qkv, self.scale).reshape(B, N, C))
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        return self.proj(F.scaled_dot_product_attention(q, k, v, scale=self.scale).transpose(1, 2).reshape(B, N, C))


class LayerScale(nn.Module):
    """layers/layer_scale.py: x * gamma."""

    def __init__(self, dim, init_values=1e-5):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Mlp(nn.Module):
    """layers/mlp.py: fc1, GELU, fc2."""

    def __init__(self, in_features, hidden_features, bias=True):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features, bias=bias)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


def _seam(x, y, ls, norm):
    """x += ls(y) in place and norm(x), one launch; (y None: the plain norm)."""
    gamma = None if y is None else (ls.gamma if isinstance(ls, LayerScale) else torch.ones_like(norm.weight))
    return ops.ls_add_layernorm(x, y, gamma, norm.weight, norm.bias, norm.eps, inplace=True)


class Block(nn.Module):
    """layers/block.py:36-107 in inference: x = x + ls1(attn(norm1(x))); x = x + ls2(mlp(norm2(x)))."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, proj_bias=True, ffn_bias=True, init_values=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, proj_bias=proj_bias)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), bias=ffn_bias)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))

    def forward_hip(self, x, h, next_norm):
        """x: the residual stream, updated in place; h = norm1(x), already formed by the seam before; next_norm: the LayerNorm that
        reads this block's result (the next block's norm1, or the model's norm).  Returns (x, next_norm(x)): two seam launches and
        one attention launch."""
        x, h = _seam(x, self.attn(h, hip=True), self.ls1, self.norm2)
        return _seam(x, self.mlp(h), self.ls2, next_norm)


class DinoVisionTransformer(nn.Module):
    """dinov2.py:43-237.  Settings the shipped model never uses raise here, naming the setting: ffn_layer other than "mlp",
    block_chunks > 0, drop_path_rate > 0.  get_intermediate_layers is not provided."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True,
                 ffn_bias=True, proj_bias=True, drop_path_rate=0.0, init_values=None, ffn_layer="mlp", block_chunks=0, impl="hip"):
        super().__init__()
        if ffn_layer != "mlp":
            raise NotImplementedError(f"DinoVisionTransformer: ffn_layer = {ffn_layer!r} is not supported, only 'mlp' (what GFNet builds)")
        if block_chunks > 0:
            raise NotImplementedError(f"DinoVisionTransformer: block_chunks = {block_chunks!r} is not supported, only 0 (what GFNet builds; "
                                      "chunking renames the blocks' parameters)")
        if drop_path_rate > 0:
            raise NotImplementedError(f"DinoVisionTransformer: drop_path_rate = {drop_path_rate!r} is not supported, only 0 (the ViT runs frozen)")
        self.impl = _check_impl(impl)
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 1
        self.n_blocks = depth
        self.num_heads = num_heads
        self.patch_size = patch_size
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + self.num_tokens, embed_dim))
        self.blocks = nn.ModuleList(Block(embed_dim, num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias,
                                          ffn_bias=ffn_bias, init_values=init_values) for _ in range(depth))
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.head = nn.Identity()
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        self.init_weights()
        for p in self.parameters():
            p.requires_grad = False
        self._pos_cache = {}

    @property
    def device(self):
        return self.cls_token.device

    def init_weights(self):
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def interpolate_pos_encoding(self, x, w, h):
        """dinov2.py:166-190, the same call: bicubic, scale_factor with the + 0.1, (w, h) in the reference's order (w is the image's
        dim 2), the early return for the native square grid.  The interpolated table is kept per grid (and per dtype, device and
        version of pos_embed, so a load_state_dict or a .to() is seen)."""
        npatch = x.shape[1] - 1
        N = self.pos_embed.shape[1] - 1
        if npatch == N and w == h:
            return self.pos_embed
        key = (w, h, x.dtype, self.pos_embed.dtype, self.pos_embed.device, self.pos_embed.data_ptr(), self.pos_embed._version)
        hit = self._pos_cache.get(key)
        if hit is not None:
            return hit
        pos_embed = self.pos_embed.float()
        class_pos_embed = pos_embed[:, 0]
        patch_pos_embed = pos_embed[:, 1:]
        dim = x.shape[-1]
        w0 = w // self.patch_size
        h0 = h // self.patch_size
        w0, h0 = w0 + 0.1, h0 + 0.1
        side = int(math.sqrt(N))
        patch_pos_embed = F.interpolate(patch_pos_embed.reshape(1, side, side, dim).permute(0, 3, 1, 2),
                                        scale_factor=(w0 / math.sqrt(N), h0 / math.sqrt(N)), mode="bicubic")
        if (int(w0), int(h0)) != tuple(patch_pos_embed.shape[-2:]):
            raise RuntimeError(f"interpolate_pos_encoding: a {int(w0)} x {int(h0)} grid was asked for, {tuple(patch_pos_embed.shape[-2:])} came out")
        patch_pos_embed = patch_pos_embed.permute(0, 2, 3, 1).reshape(1, -1, dim)
        out = torch.cat((class_pos_embed.unsqueeze(0), patch_pos_embed), dim=1).to(x.dtype)
        self._pos_cache = {k: v for k, v in self._pos_cache.items() if k[3:] == key[3:]}  # tables of an earlier pos_embed are dropped
        self._pos_cache[key] = out
        return out

    def prepare_tokens_with_masks(self, x, masks=None):
        B, nc, w, h = x.shape
        x = self.patch_embed(x)
        if masks is not None:
            x = torch.where(masks.unsqueeze(-1), self.mask_token.to(x.dtype).unsqueeze(0), x)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1)
        return x + self.interpolate_pos_encoding(x, w, h)

    def _use_hip(self, x, masks):
        _check_impl(self.impl)
        return (self.impl == "hip" and not self.training and masks is None and x.is_cuda and x.dtype in HIP_DTYPES
                and self.pos_embed.dtype == x.dtype and self.embed_dim == self.num_heads * HIP_HEAD_DIM
                and not (torch.is_grad_enabled() and x.requires_grad))

    def forward_features(self, x, masks=None):
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("DinoVisionTransformer: lists of images (nested tensors) are not supported, pass one batch")
        hip = self._use_hip(x, masks)
        x = self.prepare_tokens_with_masks(x, masks)
        if hip:
            x = x.contiguous()  # (a fresh tensor: the seams update it in place)
            _, h = _seam(x, None, None, self.blocks[0].norm1) if len(self.blocks) else _seam(x, None, None, self.norm)
            for i, blk in enumerate(self.blocks):
                x, h = blk.forward_hip(x, h, self.blocks[i + 1].norm1 if i + 1 < len(self.blocks) else self.norm)
            x_norm = h
        else:
            for blk in self.blocks:
                x = blk(x)
            x_norm = self.norm(x)
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_patchtokens": x_norm[:, 1:], "x_prenorm": x, "masks": masks}

    def forward(self, *args, is_training=False, **kwargs):
        ret = self.forward_features(*args, **kwargs)
        return ret if is_training else self.head(ret["x_norm_clstoken"])


def vit_large(patch_size=14, img_size=518, init_values=1.0, **kwargs):
    """dinov2.py:333-343 with the arguments of model/network.py:48-54 as defaults: DINOv2 ViT-L/14, width 1024, 24 blocks, 16 heads
    of 64."""
    return DinoVisionTransformer(img_size=img_size, patch_size=patch_size, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4,
                                 init_values=init_values, **kwargs)
