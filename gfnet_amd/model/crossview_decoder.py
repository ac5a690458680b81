"""The cross-view decoder between the ViT tokens and the stride-16 features, with its attention core in HIP.

A mirror, in this package's words, of the reference's `CrossVITDecoder_noself` (model/crossview_decoder_light.py:12-112) with its
`CrossBlock` (model/transformer/layers/block.py:255-329) and `CrossFlashAttention2` (model/transformer/layers/attention.py:173-258),
for the configuration every shipped config uses: attention_type "FLASH2", ffn_type "ffn", post_norm false, pre_norm_query true,
dropout 0.  Parameter names are the reference's, so the `dino_decoder.*` entries of a reference checkpoint load strictly:

    proj.weight
    cross_attn_blocks.{i}.norm1.{weight,bias}            cross_attn_blocks.{i}.attn.{q,k,v}_proj.weight
    cross_attn_blocks.{i}.attn.proj.{weight,bias}        cross_attn_blocks.{i}.ls1.gamma
    cross_attn_blocks.{i}.norm2.{weight,bias}            cross_attn_blocks.{i}.mlp.fc{1,2}.{weight,bias}
    cross_attn_blocks.{i}.ls2.gamma

The reference's attention calls flash_attn_func, which is absent on this platform (attention.py:230-231 then raises);
here it is ops.cross_attention (csrc/cross_attn.hip; ops.cross_attention_bf16 where bf16 autocast makes q, k, v bf16), and both directions of a block -- x attending to y and y to x, with the same
weights (crossview_decoder_light.py:53-54) -- are ONE launch on the concatenated batch.  attn_impl="torch" routes the core through
ops.reference_cross_attention instead: the same module on any device and dtype, which is how the tests run it in float64 on the CPU.

block_impl="torch" (the default) leaves the linear layers, LayerNorm and the MLP of a block to torch.  block_impl="hip" runs a block
in inference under fp16 or bf16 autocast as three launches on the concatenated residual stream: ops.decoder_qkv (norm1 and the q, k, v
projections, csrc/decoder_block.hip), ops.cross_attention, ops.decoder_post (output projection, both LayerScales and residual adds,
norm2 and the MLP); the entry projection and the position encoding stay torch.  Whatever that path is not built for -- train(),
tensors off the GPU, no fp16 or bf16 autocast, parameters that are not fp32, attn_impl="torch", anything that requires grad -- runs the
torch blocks, exactly as block_impl="torch" does.

train_block_impl="torch" (the default) leaves train() to those torch blocks and autograd.  train_block_impl="hip" trains the blocks
in HIP: in train() with grad mode on, on CUDA tensors under fp16 or bf16 autocast (the reference's training class,
model/network.py:171, with its amp_dtype) with fp32 parameters and the HIP attention, a block is ops.decoder_qkv_train -> ops.cross_attention -> ops.decoder_post_train on
cat(x, y), the same three forward launches (not in place) with the backward kernels of csrc/decoder_block.hip behind them; what
autograd keeps per block is X, q, k, v, the attention output and its log-sum-exp.  The entry projection, the position encoding and
the concatenation stay torch, so autograd carries the gradient on to proj.weight and the tokens.  Every other call is unchanged.
"""
import math

import torch
import torch.nn as nn

from .. import ops

ATTN_IMPLS = ("hip", "torch")
BLOCK_IMPLS = ("torch", "hip")
TRAIN_BLOCK_IMPLS = ("torch", "hip")
MAX_SHAPE = (128, 128)  # crossview_decoder_light.py:37: the extent the position encoding normalises to


def sine_position_encoding(d_model, H, W, max_shape=MAX_SHAPE):
    """(1, d_model, H, W) fp32: the normalised 2-D sine encoding of crossview_decoder_light.py:84-97.  Positions count from 1 and are
    stretched so that every grid spans max_shape; channels 4i..4i+3 are sin x, cos x, sin y, cos y at frequency
    10000^(-2i / (d_model / 2))."""
    ys = torch.arange(1, H + 1, dtype=torch.float32).view(1, H, 1).expand(1, H, W) * max_shape[0] / H
    xs = torch.arange(1, W + 1, dtype=torch.float32).view(1, 1, W).expand(1, H, W) * max_shape[1] / W
    freq = torch.exp(torch.arange(0, d_model // 2, 2).float() * (-math.log(10000.0) / (d_model // 2)))[:, None, None]
    pe = torch.zeros((d_model, H, W))
    pe[0::4], pe[1::4], pe[2::4], pe[3::4] = torch.sin(xs * freq), torch.cos(xs * freq), torch.sin(ys * freq), torch.cos(ys * freq)
    return pe.unsqueeze(0)


class LayerScale(nn.Module):
    def __init__(self, dim, init_values):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class CrossAttention(nn.Module):
    """attention.py:173-258: bias-free q/k/v projections, attention per head over the other view's tokens, output projection."""

    def __init__(self, dim, num_heads, softmax_scale=None, train_avg_length=None, attn_impl="hip"):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.softmax_scale, self.train_avg_length = softmax_scale, train_avg_length
        self.attn_impl = attn_impl
        self.q_proj = nn.Linear(dim, dim, bias=False)
        self.k_proj = nn.Linear(dim, dim, bias=False)
        self.v_proj = nn.Linear(dim, dim, bias=False)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, kv):
        B, N, C = x.shape
        h = self.num_heads
        q = self.q_proj(x).reshape(B, N, h, C // h)
        k = self.k_proj(kv).reshape(B, kv.shape[1], h, C // h)
        v = self.v_proj(kv).reshape(B, kv.shape[1], h, C // h)
        # attention.py:246-249: any softmax_scale setting selects the entropy-invariant scale, log_{train_avg_length}(N) / sqrt(d);
        # None leaves flash-attn's default 1 / sqrt(d)
        scale = self.scale if self.softmax_scale is None else self.scale * math.log(N, self.train_avg_length)
        if self.attn_impl != "hip":
            attend = ops.reference_cross_attention
        else:  # (bf16 autocast hands the projections back in bf16: the bf16 class has an op of its own name)
            attend = ops.cross_attention_bf16 if q.dtype == torch.bfloat16 else ops.cross_attention
        return self.proj(attend(q, k, v, scale).reshape(B, N, C))


class CrossBlock(nn.Module):
    """block.py:255-329 on its pre-norm branch: x + ls1(attn(norm1(x), kv)) then x + ls2(mlp(norm2(x))); the other view's tokens are
    not normalised (pre_norm_query)."""

    def __init__(self, dim, num_heads, init_values=None, softmax_scale=None, train_avg_length=None, attn_impl="hip"):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = CrossAttention(dim, num_heads, softmax_scale, train_avg_length, attn_impl)
        self.ls1 = LayerScale(dim, init_values) if init_values is not None else nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, 4 * dim)
        self.ls2 = LayerScale(dim, init_values) if init_values is not None else nn.Identity()

    def forward(self, x, kv):
        x = x + self.ls1(self.attn(self.norm1(x), kv))
        return x + self.ls2(self.mlp(self.norm2(x)))

    def forward_fused(self, X, dtype=torch.float16):
        """The block on the residual stream X = cat(x, y), (2B, N, dim) fp32, updated in place: both directions in three launches,
        in the autocast class of `dtype`, fp16 or bf16 (CrossViewDecoder._fused says when)."""
        attn, N = self.attn, X.shape[1]
        attend = ops.cross_attention_bf16 if dtype == torch.bfloat16 else ops.cross_attention
        q, k, v = ops.decoder_qkv(X, self.norm1.weight, self.norm1.bias, self.norm1.eps, attn.q_proj.weight, attn.k_proj.weight,
                                  attn.v_proj.weight, dtype=dtype)
        scale = attn.scale if attn.softmax_scale is None else attn.scale * math.log(N, attn.train_avg_length)
        # (init_values None: no LayerScale, a gamma of 1)
        gamma1, gamma2 = (ls.gamma if isinstance(ls, LayerScale) else torch.ones_like(self.norm1.weight) for ls in (self.ls1, self.ls2))
        return ops.decoder_post(X, attend(q, k, v, scale), attn.proj.weight, attn.proj.bias, gamma1, self.norm2.weight,
                                self.norm2.bias, self.norm2.eps, self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight,
                                self.mlp.fc2.bias, gamma2, inplace=True, dtype=dtype)

    def forward_train(self, X, dtype=torch.float16):
        """The block on X = cat(x, y), (2B, N, dim) fp32, differentiable and not in place: the same three launches with the HIP
        backward behind each, in the autocast class of `dtype` (CrossViewDecoder._train_fused says when).  Returns the new residual
        stream."""
        attn, N = self.attn, X.shape[1]
        attend = ops.cross_attention_bf16 if dtype == torch.bfloat16 else ops.cross_attention
        q, k, v = ops.decoder_qkv_train(X, self.norm1.weight, self.norm1.bias, self.norm1.eps, attn.q_proj.weight, attn.k_proj.weight,
                                        attn.v_proj.weight, dtype=dtype)
        scale = attn.scale if attn.softmax_scale is None else attn.scale * math.log(N, attn.train_avg_length)
        # (init_values None: no LayerScale, a constant gamma of 1 that takes no gradient)
        gamma1, gamma2 = (ls.gamma if isinstance(ls, LayerScale) else torch.ones_like(self.norm1.weight) for ls in (self.ls1, self.ls2))
        return ops.decoder_post_train(X, attend(q, k, v, scale), attn.proj.weight, attn.proj.bias, gamma1, self.norm2.weight,
                                      self.norm2.bias, self.norm2.eps, self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight,
                                      self.mlp.fc2.bias, gamma2, dtype=dtype)


def _check_cfg(cfg):
    """Raise, naming the key, for every setting of decoder_cfg whose reference behaviour is not built here."""
    supported = {"ffn_type": "ffn", "post_norm": False, "pre_norm_query": True, "attention_type": "FLASH2", "drop": 0.0, "attn_drop": 0.0,
                 "drop_path": 0.0, "mlp_ratio": 4.0, "qkv_bias": False, "proj_bias": True, "ffn_bias": True}
    for key, want in supported.items():
        value = cfg.get(key, want)  # (an absent key is the reference's default, which is the supported value for each of these)
        if value != want:
            raise NotImplementedError(f"CrossViewDecoder: decoder_cfg[{key!r}] = {value!r} is not supported, only {want!r} "
                                      "(the shipped configs' setting)")
    if cfg.get("softmax_scale") is not None and not cfg.get("train_avg_length"):
        raise ValueError("CrossViewDecoder: decoder_cfg['softmax_scale'] is set but decoder_cfg['train_avg_length'] is missing")


class CrossViewDecoder(nn.Module):
    """`decoder(x, y, vit_shape=(B, _, H, W)) -> (map_x, map_y)`: ViT patch tokens (B, H*W, d_model) of the two views -> their
    stride-16 feature maps (B, out_dim, H, W), out_dim = conf["encoder_cfg"]["feat_chs"][0] (64: 8 heads of dim 8)."""

    def __init__(self, conf, attn_impl="hip", block_impl="torch", train_block_impl="torch"):
        super().__init__()
        if attn_impl not in ATTN_IMPLS:
            raise ValueError(f"attn_impl must be one of {ATTN_IMPLS}, got {attn_impl!r}")
        if block_impl not in BLOCK_IMPLS:
            raise ValueError(f"block_impl must be one of {BLOCK_IMPLS}, got {block_impl!r}")
        if train_block_impl not in TRAIN_BLOCK_IMPLS:
            raise ValueError(f"train_block_impl must be one of {TRAIN_BLOCK_IMPLS}, got {train_block_impl!r}")
        cfg = conf["dino_cfg"]["decoder_cfg"]
        _check_cfg(cfg)
        dim = conf["encoder_cfg"]["feat_chs"][0]
        self.dim, self.attn_impl, self.block_impl, self.train_block_impl = dim, attn_impl, block_impl, train_block_impl
        self.cross_attn_blocks = nn.ModuleList(
            CrossBlock(dim, cfg["nhead"], cfg.get("init_values"), cfg.get("softmax_scale"), cfg.get("train_avg_length"), attn_impl)
            for _ in range(cfg["num_cross_attn"]))
        self.proj = nn.Linear(conf["dino_cfg"]["d_model"], dim, bias=False)
        self._pe = {}  # (H, W, device) -> (1, H*W, dim) fp32, token-major

    def position_encoding(self, H, W, device):
        key = (H, W, str(device))
        if key not in self._pe:
            self._pe[key] = sine_position_encoding(self.dim, H, W).flatten(2).transpose(1, 2).contiguous().to(device)
        return self._pe[key]

    def _train_fused(self, x, y):
        """Whether this call trains the blocks in HIP: train_block_impl="hip" with the HIP attention, train() with grad mode on,
        CUDA tensors under fp16 or bf16 autocast, fp32 parameters."""
        if self.train_block_impl != "hip" or not self.training or not torch.is_grad_enabled():
            return False
        return self._kernel_class(x, y)

    def _fused(self, x, y):
        """Whether this call takes the fused blocks: block_impl="hip" with the HIP attention, inference (eval() and nothing that
        requires grad) on CUDA tensors under fp16 or bf16 autocast with fp32 parameters -- the classes decoder_block.hip is written in."""
        if self.block_impl != "hip" or self.training or not self._kernel_class(x, y):
            return False
        return not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad or any(p.requires_grad for p in self.parameters())))

    def _kernel_class(self, x, y):
        """The classes decoder_block.hip is written in: the HIP attention, width 64, CUDA tensors under fp16 or bf16 autocast (the
        autocast dtype names the class), fp32 parameters."""
        if self.attn_impl != "hip" or not (x.is_cuda and y.is_cuda):
            return False
        if self.dim != ops.DECODER_DIM or any(b.attn.num_heads * 8 != self.dim for b in self.cross_attn_blocks):  # (the one width it is built for)
            return False
        if not torch.is_autocast_enabled("cuda") or torch.get_autocast_dtype("cuda") not in (torch.float16, torch.bfloat16):
            return False
        if any(p.dtype != torch.float32 or not p.is_cuda for p in self.parameters()):
            return False
        return True

    def forward(self, x, y, vit_shape=None):
        B, _, H, W = vit_shape
        pe = self.position_encoding(H, W, x.device)
        if x.dtype == torch.float64:
            pe = pe.double()
        fused, train_fused = self._fused(x, y), self._train_fused(x, y)
        amp = torch.get_autocast_dtype("cuda") if fused or train_fused else None  # the kernel class of this call
        x, y = self.proj(x) + pe, self.proj(y) + pe
        if train_fused and x.dtype == torch.float32:
            X = torch.cat((x, y))
            for blk in self.cross_attn_blocks:
                X = blk.forward_train(X, amp)
            x, y = X.chunk(2)
        elif fused and x.dtype == torch.float32:  # (16-bit projection + fp32 encoding: the residual stream is fp32 under autocast)
            X = torch.cat((x, y))  # the one concatenation: k and v change sides inside decoder_qkv
            for blk in self.cross_attn_blocks:
                blk.forward_fused(X, amp)
            x, y = X.chunk(2)
        else:
            for blk in self.cross_attn_blocks:
                # x against y and y against x with the same weights (crossview_decoder_light.py:53-54), as one batch of 2B
                x, y = blk(torch.cat((x, y)), torch.cat((y, x))).chunk(2)
        return (x.reshape(B, H, W, -1).permute(0, 3, 1, 2), y.reshape(B, H, W, -1).permute(0, 3, 1, 2))
