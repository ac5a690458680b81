"""Training the cross-view decoder's blocks in HIP (gfn_decoder_qkv_bwd / gfn_decoder_post_bwd in csrc/decoder_block.hip,
ops.decoder_*_bwd / ops.decoder_*_train, CrossViewDecoder's train_block_impl, ReferenceBackbone's decoder_train_impl) as far as it
goes without a GPU: the C ABI and its refusals, which return before anything is launched, the ops' refusal of CPU tensors, the
module's fallback to the torch blocks and the wiring of the backbone keyword and the environment switch."""
import ctypes

import pytest
import torch

from gfnet_amd import _lib, ops
from gfnet_amd.model.crossview_decoder import CrossViewDecoder
from test_decoder_block_cpu import _child, block_args, last_error, load_golden

vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
NEW = ("gfn_decoder_qkv_bwd", "gfn_decoder_post_bwd")


def test_abi_declares_the_backward_entry_points_with_the_headers_signatures():
    assert _lib.PROTOTYPES["gfn_decoder_qkv_bwd"] == (i32, [vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, i32, i32, i32] + [vp] * 6 + [vp, i64, vp])
    assert _lib.PROTOTYPES["gfn_decoder_post_bwd"] == (i32, [vp] * 7 + [f32] + [vp] * 6 + [i64, i32, i32] + [vp] * 12 + [vp, i64, vp])
    assert _lib.PROTOTYPES["gfn_decoder_bwd_ws_bytes"] == (i64, [i64])
    assert set(NEW) <= _lib.STATUS_FUNCS and "gfn_decoder_bwd_ws_bytes" not in _lib.STATUS_FUNCS
    assert set(NEW) | {"gfn_decoder_bwd_ws_bytes"} <= set(_lib.exported_symbols())
    L = ctypes.CDLL(_lib.LIB_PATH)  # the symbols are exported (loading the library needs no GPU)
    assert L.gfn_decoder_qkv_bwd and L.gfn_decoder_post_bwd and L.gfn_decoder_bwd_ws_bytes
    assert _lib.lib().gfn_abi_version() == 1


# a host buffer stands in for every pointer: 16-byte aligned and never read, because every call below returns before a launch
_BUF = ctypes.create_string_buffer(64)
P = ctypes.c_void_p((ctypes.addressof(_BUF) + 15) & ~15)
QKV_PTRS = ["x", "norm_weight", "norm_bias", "wq", "wk", "wv", "gq", "gk", "gv", "gx", "g_wq", "g_wk", "g_wv", "g_norm_weight", "g_norm_bias", "ws"]
POST_PTRS = ["x", "attn", "wproj", "bproj", "gamma1", "norm_weight", "norm_bias", "w1", "b1", "w2", "b2", "gamma2", "gx_out", "gx", "g_attn",
             "g_wproj", "g_bproj", "g_gamma1", "g_norm_weight", "g_norm_bias", "g_w1", "g_b1", "g_w2", "g_b2", "g_gamma2", "ws"]
BIG_WS = 1 << 40  # (never touched)


def ws_bytes(rows):
    return _lib.lib().gfn_decoder_bwd_ws_bytes(rows)


def qkv_bwd(B2=2, N=32, C=64, ptrs=None, ws=BIG_WS):
    p = [P] * 16 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_qkv_bwd(p[0], p[1], p[2], 1e-5, *p[3:9], B2, N, C, *p[9:15], p[15], ws, None)


def post_bwd(rows=32, C=64, hidden=256, ptrs=None, ws=BIG_WS):
    p = [P] * 26 if ptrs is None else ptrs
    return _lib.lib().gfn_decoder_post_bwd(*p[:7], 1e-5, *p[7:13], rows, C, hidden, *p[13:25], p[25], ws, None)


def test_unsupported_sizes_are_refused_before_anything_is_launched():
    E = _lib.ERR_INVALID_ARG
    assert qkv_bwd(C=32) == E and "C must be 64" in last_error() and "32" in last_error() and "gfn_decoder_qkv_bwd" in last_error()
    assert post_bwd(C=32) == E and "C must be 64" in last_error() and "gfn_decoder_post_bwd" in last_error()
    assert post_bwd(hidden=128) == E and "hidden width must be 256" in last_error() and "128" in last_error()
    assert qkv_bwd(B2=3) == E and "even" in last_error()
    assert qkv_bwd(N=0) == E and "bad size" in last_error()
    assert qkv_bwd(B2=-2) == E and post_bwd(rows=-1) == E
    assert qkv_bwd(B2=2 ** 16, N=2 ** 15) == E and "2^31" in last_error()


def test_null_and_misaligned_pointers_are_refused_naming_the_argument():
    E = _lib.ERR_INVALID_ARG
    off = ctypes.c_void_p(P.value + 4)
    for call, names in ((qkv_bwd, QKV_PTRS), (post_bwd, POST_PTRS)):
        for i, name in enumerate(names):
            assert call(ptrs=[None if j == i else P for j in range(len(names))]) == E
            assert "null pointer" in last_error() and f"({name})" in last_error()
            assert call(ptrs=[off if j == i else P for j in range(len(names))]) == E
            assert "16-byte aligned" in last_error() and name in last_error()


def test_the_workspace_size_is_a_function_of_the_rows_and_a_smaller_one_is_refused():
    E = _lib.ERR_INVALID_ARG
    assert ws_bytes(0) == 0 and ws_bytes(-5) == 0
    sizes = [ws_bytes(r) for r in (1, 32, 33, 2048, 67584, 10 ** 7)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] == ws_bytes(10 ** 8) < 64 << 20  # the grids stop growing: a bounded workspace
    for call, rows in ((lambda **k: qkv_bwd(B2=2, N=1024, **k), 2048), (lambda **k: post_bwd(rows=2048, **k), 2048)):
        assert call(ws=ws_bytes(rows) - 1) == E and "ws_bytes" in last_error() and "too small" in last_error()
        assert str(ws_bytes(rows)) in last_error()
        assert call(ws=0) == E


def test_an_empty_batch_is_ok_without_a_launch():
    assert qkv_bwd(B2=0, ptrs=[None] * 16, ws=0) == _lib.OK
    assert post_bwd(rows=0, ptrs=[None] * 26, ws=0) == _lib.OK


def test_cpu_tensors_raise():
    a = block_args()
    g = torch.zeros(2, 5, 8, 8, dtype=torch.float16)
    qkv = (a["X"], a["norm_weight"], a["norm_bias"], 1e-5, a["wproj"], a["wproj"], a["wproj"])
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.decoder_qkv_bwd(*qkv, g, g, g)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.decoder_post_bwd(**a, gX_out=torch.zeros_like(a["X"]))
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.decoder_qkv_train(*qkv)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.decoder_post_train(**a)
    with pytest.raises(_lib.GfnError, match="no CPU path"):  # a tensor that requires grad is no reason to refuse here
        ops.decoder_qkv_bwd(a["X"].clone().requires_grad_(), *qkv[1:], g, g, g)


def test_train_block_impl_is_checked_at_construction():
    conf = load_golden()[0]
    with pytest.raises(ValueError, match="train_block_impl"):
        CrossViewDecoder(conf, train_block_impl="cudnn")
    assert CrossViewDecoder(conf).train_block_impl == "torch"  # the default: every existing construction is what it was
    dec = CrossViewDecoder(conf, attn_impl="torch", train_block_impl="hip")
    assert dec.train_block_impl == "hip" and dec.block_impl == "torch"


def test_train_block_impl_hip_on_the_cpu_gives_the_torch_blocks_gradients_bit_for_bit():
    conf, state, x, y, _, (B, H, W), _ = load_golden()
    grads = {}
    for impl in ("hip", "torch"):
        dec = CrossViewDecoder(conf, attn_impl="torch", train_block_impl=impl)
        dec.load_state_dict(state, strict=True)
        dec.train()
        xs, ys = x.clone().requires_grad_(), y.clone().requires_grad_()
        assert not dec._train_fused(xs, ys)
        mx, my = dec(xs, ys, vit_shape=(B, 3, H, W))
        (mx.square().sum() + (my * mx.detach()).sum()).backward()
        grads[impl] = {"x": xs.grad, "y": ys.grad, **{k: p.grad for k, p in dec.named_parameters()}}
    assert set(grads["hip"]) == set(grads["torch"]) and len(grads["hip"]) > 10
    for k, g in grads["hip"].items():
        assert g is not None and float(g.abs().max()) > 0 and torch.equal(g, grads["torch"][k]), k


def test_wiring_decoder_train_impl_reaches_the_native_decoder_and_is_refused_for_the_checkouts(tmp_path):
    _child("""
    bb = compat.reference_backbone(conf, vit=vit, decoder="hip_fused", decoder_train_impl="hip")
    assert type(bb.dino_decoder) is CrossViewDecoder
    assert bb.dino_decoder.train_block_impl == "hip" and bb.dino_decoder.block_impl == "hip"
    assert compat.reference_backbone(conf, vit=vit, decoder="hip", decoder_train_impl="hip").dino_decoder.train_block_impl == "hip"
    assert compat.reference_backbone(conf, vit=vit, decoder="hip").dino_decoder.train_block_impl == "torch"  # the default
    assert "model.crossview_decoder_light" not in sys.modules
    for kw, msg in ((dict(decoder="checkout", decoder_train_impl="hip"), "needs decoder="), (dict(decoder_train_impl="hip"), "needs decoder="),
                    (dict(decoder="hip", decoder_train_impl="cudnn"), "must be 'torch' or 'hip'")):
        try:
            compat.reference_backbone(conf, vit=vit, **kw)
        except ValueError as e:
            assert msg in str(e), e
        else:
            raise AssertionError(kw)
    print("ok")
    """, tmp_path)


def test_wiring_environment_switch_selects_the_hip_training_blocks(tmp_path):
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    model = GFNet(conf=conf)
    dec = model.backbone.dino_decoder
    assert type(dec) is CrossViewDecoder and dec.block_impl == "hip" and dec.train_block_impl == "hip"
    print("ok")
    """, tmp_path, env={"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip_fused", "GFNET_COMPAT_DECODER_TRAIN": "hip"})


def test_wiring_without_the_switch_the_blocks_train_through_torch(tmp_path):
    _child("""
    import gfnet_amd.reference_backbone as rb
    rb._build_vit = lambda w: vit
    from model.network import GFNet
    assert GFNet(conf=conf).backbone.dino_decoder.train_block_impl == "torch"
    print("ok")
    """, tmp_path, env={"GFNET_COMPAT_BACKBONE": "reference", "GFNET_COMPAT_DECODER": "hip_fused"})
