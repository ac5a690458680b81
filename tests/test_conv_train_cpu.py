"""Training-mode conv block without a GPU: the host checks of gfn_conv_block_train_fwd / _bwd (csrc/conv_stack_train.hip) and the
register budget of their kernels -- what tests/test_conv_train_gpu.py runs on the device."""
import ctypes
import os
import subprocess
import sys

from conftest import ROOT


def test_conv_block_train_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every call below has exactly one bad argument and must be refused by the host checks, before a launch (every pointer is a
    host buffer that no kernel may ever see; the workspace it claims is large enough, so only the argument under test can refuse)."""
    from gfnet_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    q, r = ctypes.c_void_p(p.value + 16), ctypes.c_void_p(p.value + 32)   # x, u and y must differ
    BIG = 1 << 40

    def fwd(x=p, dw_w=p, dw_b=p, bn_w=p, bn_b=p, rm=p, rv=p, pw_w=p, pw_b=p, u=q, mean=p, invstd=p, y=r, B=2, C=24, M=24, G=16,
            momentum=0.1, eps=1e-5, ws=p, nws=BIG):
        return L.gfn_conv_block_train_fwd(x, dw_w, dw_b, bn_w, bn_b, rm, rv, pw_w, pw_b, u, mean, invstd, y, B, C, M, G, momentum, eps, ws,
                                          nws, None)

    def bwd(gy=p, x=p, u=p, mean=p, invstd=p, dw_w=p, bn_w=p, bn_b=p, pw_w=p, gx=p, d_dw_w=p, d_dw_b=p, d_bn_w=p, d_bn_b=p, d_pw_w=p,
            d_pw_b=p, B=2, C=24, M=24, G=16, need=15, ws=p, nws=BIG):
        return L.gfn_conv_block_train_bwd(gy, x, u, mean, invstd, dw_w, bn_w, bn_b, pw_w, gx, d_dw_w, d_dw_b, d_bn_w, d_bn_b, d_pw_w, d_pw_b,
                                          B, C, M, G, need, ws, nws, None)

    def refused(code, what, scratch=False):
        assert code == (-3 if scratch else -1), what
        assert L.gfn_last_error(), what

    need_fwd = int(L.gfn_conv_block_train_ws_bytes(2, 24, 24, 16, 0))
    need_bwd = int(L.gfn_conv_block_train_ws_bytes(2, 24, 24, 16, 1))
    # forward: one 32x32 tile per 16x16 map, (mean, M2) per tile and channel
    assert need_fwd == 24 * 2 * 1 * 2 * 4
    assert need_bwd > 2 * 24 * 256 * 4                      # at least the gz map
    assert L.gfn_conv_block_train_ws_bytes(0, 24, 24, 16, 1) == 0 and L.gfn_conv_block_train_ws_bytes(2, 0, 24, 16, 0) == 0

    for name in ("x", "dw_w", "bn_w", "bn_b", "rm", "rv", "pw_w", "pw_b", "u", "mean", "invstd", "y"):
        refused(fwd(**{name: None}), f"fwd: null {name}")
    for what, kw in {"C = 0": dict(C=0), "C < 0": dict(C=-3), "M = 0": dict(M=0), "G = 0": dict(G=0), "B < 0": dict(B=-1),
                     "a map of 2^29 floats": dict(C=1 << 13, G=1 << 8), "batch > 65535": dict(B=65536), "u aliases x": dict(u=p),
                     "y aliases u": dict(y=q), "one value per channel": dict(B=1, G=1), "momentum > 1": dict(momentum=1.5),
                     "negative eps": dict(eps=-1.0)}.items():
        refused(fwd(**kw), "fwd: " + what)
    for what, kw in {"null workspace": dict(ws=None), "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 4)),
                     "workspace too small": dict(nws=need_fwd - 1)}.items():
        refused(fwd(**kw), "fwd: " + what, scratch=True)
    assert fwd(B=0) == 0                                     # nothing to compute: valid, and no launch

    for name in ("gy", "x", "u", "mean", "invstd", "dw_w", "bn_w", "bn_b", "pw_w"):
        refused(bwd(**{name: None}), f"bwd: null {name}")
    for what, kw in {"C = 0": dict(C=0), "M < 0": dict(M=-1), "G = 0": dict(G=0), "B < 0": dict(B=-1), "need = 16": dict(need=16),
                     "need < 0": dict(need=-1), "need x without gx": dict(gx=None), "need dw without d_dw_w": dict(d_dw_w=None),
                     "need bn without d_bn_b": dict(d_bn_b=None), "need pw without d_pw_w": dict(d_pw_w=None)}.items():
        refused(bwd(**kw), "bwd: " + what)
    for what, kw in {"null workspace": dict(ws=None), "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 8)),
                     "workspace too small": dict(nws=need_bwd - 1)}.items():
        refused(bwd(**kw), "bwd: " + what, scratch=True)
    # nothing to compute: an empty batch or an empty need mask; a block without depthwise bias passes no d_dw_b
    assert bwd(B=0) == 0 and bwd(need=0) == 0 and bwd(need=0, d_dw_b=None, gx=None) == 0


def assert_train_kernels_have_no_spills_and_no_scratch(obj_name, count):
    """Every training kernel of csrc/<obj_name> -- both classes name theirs ct_... -- has no VGPR or SGPR spill, no scratch and at
    most 64 KiB of LDS, and there are exactly `count` of them (tests/test_conv_train_amp_cpu.py checks the fp16 class's object)."""
    obj = os.path.join(ROOT, "gfnet_amd", "csrc", obj_name)
    if not os.path.exists(obj):
        from gfnet_amd import build

        build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj, "ct_"], capture_output=True, text=True,
                         check=True).stdout
    rows = [ln for ln in out.splitlines() if "ct_" in ln]
    assert len(rows) == count, out
    for ln in rows:
        f = ln.split()
        vals = {f[k]: f[k + 1] for k in range(len(f) - 1) if f[k] in ("spill", "sspill", "scratch")}
        assert vals == {"spill": "0", "sspill": "0", "scratch": "0"}, ln
        lds = int(f[f.index("lds") + 1])
        assert lds <= 64 * 1024, ln


def test_conv_block_train_kernels_have_no_spills_and_no_scratch():
    # 6 plain kernels (the depthwise pair is one instantiation each) + the 1x1 forward and backward for 1..7 row tiles + 8 shapes of
    # the 1x1 weight gradient
    assert_train_kernels_have_no_spills_and_no_scratch("conv_stack_train.o", 6 + 7 + 7 + 8)


def test_train_conv_impl_defaults_to_torch_and_leaves_the_eval_predicate_alone():
    from gfnet_amd.model.network import ConvRefiner

    ref = ConvRefiner(24, 24, 3, dw=True, hidden_blocks=2, displacement_emb="linear", displacement_emb_dim=8, local_corr_num=0,
                      corr_in_other=False)
    assert ref.train_conv_impl == "torch"
    ref.train_conv_impl = "hip"
    ref.train()
    assert not ref._hip_stack_supported()
