"""CPU-side checks: the C-ABI library loads and exports every symbol include/gfnet_hip.h declares
(no compute calls without a GPU), host logic of the estimation mirror against the goldens, the
network mirror's parameter layout against the reference's state_dict keys, the no-CPU-fallback rule."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def test_library_exports_every_declared_symbol():
    from gfnet_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "gfnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gfn_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in include/gfnet_hip.h but not exported"
    # the binding's parser against this test's own scan of the names: a prototype it skipped would show here
    assert declared == set(_lib.exported_symbols()), declared ^ set(_lib.exported_symbols())
    # and the library itself: its defined dynamic gfn_* symbols are exactly the declared ones, in both directions
    syms = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--dyn-syms", "-W", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {f[7].split("@")[0] for f in (ln.split() for ln in syms.splitlines()) if len(f) == 8 and f[6] != "UND" and f[7].startswith("gfn_")}
    assert defined == declared, defined ^ declared
    assert L.gfn_abi_version() == 1


def test_argument_errors_return_codes_without_a_gpu():
    from gfnet_amd import _lib

    L = _lib.lib()
    # null pointers / bad sizes are rejected before anything touches the device
    assert L.gfn_local_corr_fwd(None, 0, None, None, None, None, 0, 1, 16, 4, 8, 8, 2, 0, 8, 8, None, 0, None) == -1
    assert b"null" in L.gfn_last_error()
    assert L.gfn_interp_bilinear_fwd(None, None, 1, 2, 2, 2, 2, None) == -1
    assert L.gfn_kde_msplit(1, 20000, 20000) >= 1
    assert L.gfn_homography_scratch_bytes(2, 100) >= 2 * 100 * 76


def test_corr_entry_points_refuse_bad_arguments_without_a_gpu():
    """csrc/corr_softargmax.hip: every call below has exactly one bad argument and must be refused by the host checks, before a
    launch (the feature / output pointers are a host buffer that no kernel may ever see)."""
    import ctypes

    from gfnet_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    F32, F16 = _lib.GFN_F32, _lib.GFN_F16

    def refused(code, what):
        assert code == -1, what
        assert L.gfn_last_error(), what

    def fused(f0=p, f1=p, flow=p, B=2, C=16, H0=4, W0=4, H1=4, W1=4, sym=0):
        """every fused entry point and dtype with the same arguments"""
        yield L.gfn_corr_softargmax_fwd(f0, f1, flow, B, C, H0, W0, H1, W1, sym, None)
        for dt in (F32, F16):
            yield L.gfn_corr_softargmax_fwd_dt(f0, f1, dt, flow, B, C, H0, W0, H1, W1, sym, None)
            yield L.gfn_corr_softargmax_fwd_ws(f0, f1, dt, flow, B, C, H0, W0, H1, W1, sym, p, 64, None)
            yield L.gfn_corr_softargmax_fwd_ws(f0, f1, dt, flow, B, C, H0, W0, H1, W1, sym, None, 0, None)

    def volume(f0=p, f1=p, vol=p, flow=p, B=2, C=16, H0=4, W0=4, H1=4, W1=4):
        yield L.gfn_corr_volume_fwd(f0, f1, vol, flow, B, C, H0, W0, H1, W1, None)
        yield L.gfn_corr_volume_fwd(f0, f1, vol, None, B, C, H0, W0, H1, W1, None)

    bad = {"C = 0": dict(C=0), "C = 129": dict(C=129), "B < 0": dict(B=-1), "null f0": dict(f0=None), "null f1": dict(f1=None),
           "H0 = 0": dict(H0=0), "W1 = 0": dict(W1=0), "A map of 2^24 positions": dict(H0=4096, W0=4096),
           "B map of 2^24 positions": dict(H1=1, W1=1 << 24), "B map of 2^24 + 2^12 positions": dict(H1=4097, W1=4096)}
    for what, kw in bad.items():
        for code in fused(**kw):
            refused(code, what)
        for code in volume(**kw):
            refused(code, what)
    for what, kw in {"symmetric, odd batch": dict(B=3, sym=1), "symmetric, unequal widths": dict(W1=5, sym=1),
                     "symmetric, unequal heights": dict(H0=5, sym=1), "null flow": dict(flow=None)}.items():
        for code in fused(**kw):
            refused(code, what)
    for code in volume(vol=None):
        refused(code, "null volume")
    refused(L.gfn_corr_softargmax_fwd_dt(p, p, 7, p, 2, 16, 4, 4, 4, 4, 0, None), "unknown dtype")
    refused(L.gfn_corr_softargmax_fwd_ws(p, p, 7, p, 2, 16, 4, 4, 4, 4, 0, None, 0, None), "unknown dtype")
    for args in [(None, p, 1, 4, 4, 4, 4), (p, None, 1, 4, 4, 4, 4), (p, p, -1, 4, 4, 4, 4), (p, p, 1, 0, 4, 4, 4), (p, p, 1, 4, 4, 4, 0)]:
        refused(L.gfn_pos_embed_fwd(*args, None), f"pos_embed {args[2:]}")
    # an empty batch is valid and returns before any launch
    assert all(code == 0 for code in fused(B=0)) and all(code == 0 for code in volume(B=0))
    assert L.gfn_pos_embed_fwd(p, p, 0, 4, 4, 4, 4, None) == 0


def test_kde_entry_points_refuse_bad_arguments_without_a_gpu():
    """csrc/kde.hip: every call below has exactly one bad argument and must be refused by the host checks before any launch (all
    pointers are host buffers that no kernel may ever see)."""
    import ctypes

    from gfnet_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)  # 16-byte aligned / float aligned only
    INVALID, SCRATCH = -1, -3
    nan = float("nan")

    def density(x=p, y=p, out=p, Bt=1, N=8, M=8, D=4, rs=4, bs=32, std=0.1, scratch=None, n=0):
        return L.gfn_kde_density(x, y, out, Bt, N, M, D, rs, bs, std, scratch, n, None)

    for what, kw in {"std = 0": dict(std=0.0), "std < 0": dict(std=-0.1), "std NaN": dict(std=nan), "row stride < D": dict(rs=3),
                     "row stride < D = 5": dict(D=5, rs=4), "Bt > 65535": dict(Bt=65536), "D = 0": dict(D=0), "N < 0": dict(N=-1),
                     "M < 0": dict(M=-1), "null x": dict(x=None), "null y": dict(y=None), "null out": dict(out=None)}.items():
        assert density(**kw) == INVALID, what
        assert L.gfn_last_error(), what
    assert density(Bt=0) == 0 and density(N=0) == 0  # empty: valid, returns before any launch

    need = int(L.gfn_kde_sorted_scratch_floats(1, 8, 8))

    def dsorted(x=p, y=p, out=p, perm=None, Bt=1, N=8, M=8, std=0.1, scratch=p, n=None):
        return L.gfn_kde_density_sorted(x, y, out, perm, Bt, N, M, std, 0, scratch, need if n is None else n, None)

    for what, kw in {"std = 0": dict(std=0.0), "std < 0": dict(std=-1.0), "std NaN": dict(std=nan), "M = 0": dict(M=0), "M < 0": dict(M=-5),
                     "N < 0": dict(N=-1), "Bt > 65535": dict(Bt=65536), "null x": dict(x=None), "null y": dict(y=None),
                     "null out": dict(out=None), "null scratch": dict(scratch=None),
                     "std below the matrix-core domain": dict(std=0.06), "std far below": dict(std=0.01)}.items():
        assert dsorted(**kw) == INVALID, what
        assert L.gfn_last_error(), what
    assert b"std" in L.gfn_last_error()
    for what, kw in {"misaligned x": dict(x=odd), "misaligned scratch": dict(scratch=odd), "scratch one float short": dict(n=need - 1),
                     "no scratch floats": dict(n=0)}.items():
        assert dsorted(**kw) == SCRATCH, what
    assert dsorted(Bt=0, n=int(L.gfn_kde_sorted_scratch_floats(0, 8, 8))) == 0 and dsorted(N=0) == 0
    assert dsorted(std=0.0625, N=0) == 0  # the edge of the domain is inside it

    def msort(x=p, xs=p, perm=p, scratch=p, Bt=1, N=8):
        return L.gfn_kde_morton_sort(x, xs, perm, scratch, Bt, N, None)

    for what, kw in {"row longer than 65535 * 16": dict(N=65535 * 16 + 1), "misaligned x": dict(x=odd), "misaligned x_sorted": dict(xs=odd),
                     "null perm": dict(perm=None), "null scratch": dict(scratch=None), "null x": dict(x=None), "Bt < 0": dict(Bt=-1),
                     "N < 0": dict(N=-1)}.items():
        assert msort(**kw) == INVALID, what
    assert b"too long" in (L.gfn_kde_morton_sort(p, p, p, p, 1, 65535 * 16 + 1, None), L.gfn_last_error())[1]
    assert msort(Bt=0) == 0 and msort(N=0) == 0
    assert L.gfn_kde_morton_keys(odd, p, 4, None) == INVALID and L.gfn_kde_morton_keys(None, p, 4, None) == INVALID
    assert L.gfn_kde_morton_keys(p, None, 4, None) == INVALID and L.gfn_kde_morton_keys(p, p, -1, None) == INVALID
    assert L.gfn_kde_morton_keys(p, p, 0, None) == 0


def test_kde_sorted_scratch_covers_the_carve_up():
    """gfn_kde_sorted_scratch_floats against the carve-up of gfn_kde_density_sorted, recomputed here (offsets in floats): pre-scaled
    x and point pairs, 64- and 32-point boxes, up to 32 split-M partials, the bf16x8 operand images (16 bytes per entry, 128 per
    64-row / 64-column tile pair), the 64-bit column sums.  Every region 16-byte aligned where the kernels read vectors, the last
    byte inside the buffer, for every edge size and the production call."""
    from gfnet_amd import _lib

    L = _lib.lib()
    sizes = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 10000]
    for Bt in (1, 3, 32):
        for N in sizes:
            for M in {N, 1, 63, 333, 4097, sizes[(sizes.index(N) + 5) % len(sizes)]}:
                Mp = (M + 1) & ~1
                nblk = (Mp + 63) // 64
                NT, MT = (N + 63) // 64 * 2, nblk * 2
                xs = 0
                ys = xs + Bt * N * 4
                box = ys + Bt * Mp * 4
                box32 = box + ((Bt * nblk * 8 + 3) & ~3)
                part = box32 + Bt * nblk * 16
                aop = part + ((Bt * 32 * N + 3) & ~3)       # room for MS = 32 partial rows
                bop = aop + Bt * NT * 128 * 4
                colacc = bop + Bt * MT * 128 * 4
                end = colacc + Bt * N * 2
                assert all(o % 4 == 0 for o in (ys, box, box32, part, aop, bop)) and colacc % 2 == 0, (Bt, N, M)
                assert end <= int(L.gfn_kde_sorted_scratch_floats(Bt, N, M)), (Bt, N, M)
                # the split never exceeds the 32 partial rows the carve-up leaves room for
                blocks, ms = Bt * ((N + 255) // 256), 1
                while blocks * ms < 2048 and nblk // (ms * 2) >= 8 and ms < 32:
                    ms *= 2
                assert ms <= 32


def test_corr_general_loop_row_index_is_exact_below_2_pow_24():
    """corr_softargmax_kernel's general loop turns a B-position j into (jx, jy) with a float quotient and one integer correction
    step (csrc/corr_softargmax.hip).  This is that formula in float32 / int32 arithmetic, with inv_w1 = 1.0f / W1 correctly rounded,
    for every j below check_args' 2^24 limit.  The quotient alone is a row too high at some j >= 2^22 (W1 = 4095: x = W1 - 2,
    W1 - 1 from row 1025 on), which put a B-position at x = -1 or -2 of the next row."""
    j = np.arange(1 << 24, dtype=np.int32)
    jf = j.astype(np.float32) + np.float32(0.5)
    for W1 in (1, 2, 3, 5, 31, 33, 63, 65, 80, 1000, 4095, 4096, 65535, (1 << 24) - 1):
        inv_w1 = np.float32(1.0) / np.float32(W1)
        jy = (jf * inv_w1).astype(np.int32)                  # (int)(((float)j + 0.5f) * inv_w1): a float32 product, truncated
        jx = j - jy * np.int32(W1)
        if W1 in (1, 3, 63, 4095, 65535):
            assert (jx < 0).any()                            # the float quotient alone is wrong here ...
        assert jx.min() >= -W1 and jx.max() < 2 * W1         # ... by at most one row either way, which one step corrects
        lo, hi = jx < 0, jx >= W1
        jy[lo] -= 1
        jx[lo] += W1
        jy[hi] += 1
        jx[hi] -= W1
        assert np.array_equal(jy, j // W1), W1
        assert np.array_equal(jx, j % W1), W1


def test_product_ops_refuse_cpu_tensors():
    from gfnet_amd import ops
    from gfnet_amd._lib import GfnError
    from gfnet_amd.utils.kde import kde

    with pytest.raises(GfnError):
        ops.corr_softargmax(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4))
    with pytest.raises(GfnError):
        kde(torch.zeros(16, 4), half=False)
    with pytest.raises(GfnError):
        ops.find_homography(torch.zeros(1, 10, 4))


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gfnet_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "liboracle" in src:
                    bad.append(f)
    assert not bad, bad


def test_estimation_mirror_against_goldens():
    from gfnet_amd import estimation as E

    g = load_golden("g8_estimation")
    np.testing.assert_allclose(E.auc(list(g["errors"]), [3, 5, 10, 20]), g["aucs"], rtol=1e-12)
    np.testing.assert_allclose(E.auc(list(g["errors_few"]), [3, 5, 10, 20]), g["aucs_few"], rtol=1e-12)
    wq, hq, ws, hs = [int(v) for v in g["conv_sizes"]]
    pa, pb = E.convert_coordinates(g["conv_a"], g["conv_b"], wq, hq, ws, hs)
    np.testing.assert_array_equal(pa, g["conv_pa"])
    np.testing.assert_array_equal(pb, g["conv_pb"])
    ta, tb = E.convert_coordinates(torch.from_numpy(g["conv_a"]), torch.from_numpy(g["conv_b"]), wq, hq, ws, hs)
    np.testing.assert_allclose(ta.numpy(), g["conv_pa"], rtol=1e-6)
    w1, h1, _, _ = [int(v) for v in g["demo.sizes"]]
    for tag in ("near", "far"):
        assert abs(E.corner_error(g["demo.H_gt"], g[f"demo.{tag}.H_pred"], w1, h1) - float(g[f"demo.{tag}.ace"])) < 1e-9
    # failed solve: diag(0,0,1) -> the reference's value for that case
    ace_none = E.corner_error(g["demo.H_gt"], np.diag([0.0, 0.0, 1.0]), w1, h1)
    ref = float(g["demo.none.ace"])
    assert (np.isnan(ref) and np.isnan(ace_none)) or abs(ace_none - ref) < 1e-9


def test_refiner_parameter_layout_matches_reference_state_dict():
    from gfnet_amd.model.network import ConvRefiner

    g = load_golden("g4_refiner_prefix")
    c, disp, r = 8, 6, 2
    dim = 2 * c + disp + (2 * r + 1) ** 2
    ref = ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=2, displacement_emb="linear",
                      displacement_emb_dim=disp, local_corr_num=r, corr_in_other=True, amp=True, bn_momentum=0.01)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    missing, unexpected = ref.load_state_dict(sd, strict=True)
    assert not missing and not unexpected


def test_gfnet_builds_from_basic_config_shapes():
    from gfnet_amd.model.network import GFNet

    conf = {"encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
            "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0],
                        "displacement_dim": [64, 64, 32, 16, 8], "num_itr": [1, 1, 1, 1, 1]}}  # gfnet_configs/basic.json:19-27
    m = GFNet(conf, symmetric=True, upsample_preds=True, attenuate_cert=True)
    # input widths of the five refiners (network.py:79-154): 2c + disp + (2r+1)^2
    assert [m.conv_refiner[s].block1[0].in_channels for s in ("16", "8", "4", "2", "1")] == [417, 361, 177, 73, 24]
    assert m.upsample_grids(560) == ([40, 80, 160, 320], [6, 4, 2, 0], [1, 1, 1, 1])
    with pytest.raises(NotImplementedError):
        m.extract_features(torch.zeros(2, 3, 448, 448))


def test_concat_tensor_is_reused_only_outside_autograd_graphs():
    """the second iteration at a scale overwrites the previous concat tensor `d` in place through raw pointers.
    That is only allowed when `d` cannot be saved for a backward pass: grad mode off, or nothing upstream / in the refiner
    asks for gradients.  The slot is the caller's (a list handed through forward), never module state."""
    import torch

    from gfnet_amd.model.network import ConvRefiner

    ref = ConvRefiner(24, 24, 3, kernel_size=5, dw=True, hidden_blocks=1, displacement_emb="linear", displacement_emb_dim=4,
                      local_corr_num=0, corr_in_other=False)
    x, y, flow = torch.zeros(1, 10, 4, 4), torch.zeros(1, 10, 4, 4), torch.zeros(1, 2, 4, 4)
    assert not hasattr(ref, "last_d")
    with torch.no_grad():
        assert ref.may_reuse_d(x, y, flow)
    assert not ref.may_reuse_d(x, y, flow)              # trainable conv blocks: block1 would save d
    for p in ref.parameters():
        p.requires_grad_(False)
    assert ref.may_reuse_d(x, y, flow)                  # frozen refiner, detached inputs
    assert not ref.may_reuse_d(x, y, flow.clone().requires_grad_(True))
    ref.out_conv.weight.requires_grad_(True)
    assert not ref.may_reuse_d(x, y, flow)


def test_product_kernels_keep_their_register_budget():
    """spills of the product kernels are tracked, not discovered.  From the metadata of the built objects
    (tools/kernel_regs.py): the fp32 instantiations of the default local-correlation paths stay spill-free where they are today
    (lean r <= 2, the r >= 5 matrix-core kernel), the known exceptions stay bounded -- the lean r = 3 / 4 kernels carry the
    second-launch worker path (<= 80 spilled registers, all in the worker branch: round 5 built the same kernels without the
    worker: no spills and no scratch, csrc/local_corr_lean.h; it measured the separate launch 12 us slower under the
    bench's flows and kept the inlined form).  The fp16 instantiations of the r >= 5 kernels (pyramids
    stored in fp16, BASELINE configs[4]) spilled 16-39 registers until round 4: the choice between the two staging forms was a run-time
    flag for fp16 maps (even / odd width) and both forms' load registers were live at once; it is a template parameter now (QOK) and
    the even-width instantiations sit at 78-105 registers, the odd-width ones at <= 128 with at most one spill."""
    import re
    import subprocess
    import sys

    obj = os.path.join(ROOT, "gfnet_amd", "csrc", "local_corr.o")
    if not os.path.exists(obj):
        pytest.skip("local_corr.o not built (python -m gfnet_amd.build)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.splitlines():
        m = re.search(r"(local_corr_\w+?)(?:I|<)(.*?)\s+vgpr\s+(\d+) spill\s+(\d+).*?scratch\s+(\d+)", line)
        if not m:
            continue
        name, rest, vgpr, spill, scratch = m.group(1), line, int(m.group(3)), int(m.group(4)), int(m.group(5))
        half = "DF16_" in rest or "_Float16" in rest
        if "tile2_kernel" in name:
            r = int(re.search(r"tile2_kernel(?:ILi|<)(\d)", rest).group(1))
            seen += 1
            if r <= 2:
                assert spill <= 1 and vgpr <= 80, line          # three workgroups per CU
            else:
                assert spill <= 80 and scratch <= 330 and vgpr <= 128, line        # the worker branch's spills
        elif "mq_kernel" in name:
            seen += 1
            assert vgpr <= 128, line
            assert spill <= (1 if half else 0), line
        elif name.endswith("local_corr_tile_kernel") or "local_corr_tile_kernel" in name and "tile2" not in name:
            r = int(re.search(r"tile_kernel(?:ILi|<)(\d)", rest).group(1))
            if r >= 5:
                seen += 1
                assert vgpr <= 128 and spill == 0, line  # two workgroups of eight waves per CU
    assert seen >= 12
    # the matrix-core KDE kernels (0.35 ms of a 448b32 step): no spills in either form (round 6: the symmetric one carried the five
    # permute indices of its final butterfly across the main loop in scratch)
    kobj = os.path.join(ROOT, "gfnet_amd", "csrc", "kde.o")
    kout = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), kobj, "kde4_mfma_kernel"], capture_output=True, text=True,
                          check=True).stdout
    klines = [ln for ln in kout.splitlines() if "kde4_mfma_kernel" in ln]
    assert len(klines) >= 2
    for ln in klines:
        m = re.search(r"vgpr\s+(\d+) spill\s+(\d+).*?scratch\s+(\d+)", ln)
        assert int(m.group(1)) <= 128 and int(m.group(2)) == 0 and int(m.group(3)) == 0, ln


def test_compat_directory_resolves_the_reference_imports():
    """with compat/ in front on sys.path the reference's own import lines (test.py:9-11, model/network.py:10-11)
    bind to gfnet_amd -- in a child process, so that this process's `utils` / `model` modules are not disturbed."""
    import subprocess
    import sys

    code = ("from model.network import GFNet; from estimation import demo_estimation, auc; "
            "from utils.local_correlation import local_correlation; from utils.kde import kde; "
            "import gfnet_amd.model.network as n, gfnet_amd.estimation as e, gfnet_amd.utils.local_correlation as l, gfnet_amd.utils.kde as k; "
            "assert GFNet is n.GFNet and demo_estimation is e.demo_estimation and auc is e.auc; "
            "assert local_correlation is l.local_correlation and kde is k.kde; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_gfnet_loads_a_full_reference_checkpoint():
    """test.py:37-38 hands load_state_dict the whole `states["model"]`: conv_refiner.* entries load, the reference's backbone entries
    (dino_decoder / encoder / decoder / merge_layer, network.py:47-60) are set aside without a backbone module and routed into one
    that has them; an unknown key is still an error under strict=True."""
    import torch.nn as nn

    from gfnet_amd.model.network import GFNet

    conf = {"encoder_cfg": {"feat_chs": [64, 32, 16, 8]},
            "matcher": {"num_grid": [32, 32, 64, 128, 256], "radius": [7, 6, 4, 2, 0],
                        "displacement_dim": [64, 64, 32, 16, 8], "num_itr": [1, 1, 1, 1, 1]}}
    torch.manual_seed(3)
    src = GFNet(conf)
    ckpt = {k: v + 1.0 if v.is_floating_point() else v for k, v in src.state_dict().items()}
    ckpt.update({"encoder.layer0.weight": torch.ones(4, 4), "decoder.up.bias": torch.zeros(4), "dino_decoder.blocks.0.w": torch.zeros(2),
                 "merge_layer.0.weight": torch.full((3,), 2.0)})
    dst = GFNet(conf, initial_res=(448, 448), upsample_res=(560, 560), symmetric=True, upsample_preds=True, attenuate_cert=True)
    assert dst.initial_res == (448, 448)
    res = dst.load_state_dict(ckpt)  # strict
    assert not res.missing_keys and not res.unexpected_keys
    assert sorted(dst.ignored_backbone_keys) == ["decoder.up.bias", "dino_decoder.blocks.0.w", "encoder.layer0.weight", "merge_layer.0.weight"]
    for k, v in dst.state_dict().items():
        assert torch.equal(v, ckpt[k]), k

    class Backbone(nn.Module):  # a wrapper with (some of) the reference's submodule names
        def __init__(self):
            super().__init__()
            self.merge_layer = nn.Sequential(nn.BatchNorm1d(3))

        def forward(self, x, upsample=False):
            raise NotImplementedError

    dst2 = GFNet(conf, backbone=Backbone())
    dst2.load_state_dict(ckpt, strict=False)
    assert torch.equal(dst2.backbone.merge_layer[0].weight, torch.full((3,), 2.0))
    assert "merge_layer.0.weight" not in dst2.ignored_backbone_keys
    with pytest.raises(RuntimeError):
        dst.load_state_dict(dict(ckpt, bogus=torch.zeros(1)))


def test_refiner_keeps_the_flags_the_reference_stores_without_reading_them():
    """The reference's ConvRefiner takes no_im_B_fm / concat_logits / use_cosine_corr / disable_local_corr_grad / is_classifier, stores
    them (network.py:496-501) and its forward (network.py:533-564) never reads one of them.  The mirror does the same: a constructor call
    written for the reference builds the same module, the flags are attributes without effect (rounds 1-4 raised NotImplementedError)."""
    from gfnet_amd.model.network import ConvRefiner

    kw = dict(dw=True, hidden_blocks=1, displacement_emb="linear", displacement_emb_dim=2, local_corr_num=1, corr_in_other=True)
    torch.manual_seed(0)
    plain = ConvRefiner(10, 10, 3, **kw)
    torch.manual_seed(0)
    flagged = ConvRefiner(10, 10, 3, no_im_B_fm=True, concat_logits=True, use_cosine_corr=True, disable_local_corr_grad=True, is_classifier=True, **kw)
    assert flagged.no_im_B_fm and flagged.concat_logits and flagged.use_cosine_corr and flagged.disable_local_corr_grad and flagged.is_classifier
    assert list(plain.state_dict()) == list(flagged.state_dict())
    for (k, a), b in zip(plain.state_dict().items(), flagged.state_dict().values()):
        assert torch.equal(a, b), k


def test_refiner_input_wave_mapping_is_a_permutation_of_the_cells():
    """csrc/refiner_input.h (round 6): thread index -> cell so that a wave covers 2 grid rows x 32 columns.  The kernel's integer
    expressions restated: every cell of a direction is visited exactly once, a wave's 64 threads form the block, and grids that are not
    a multiple of 32 keep the linear order."""
    import numpy as np

    def remap(cell, G):
        if G % 32:
            return cell
        w, lane, wpr = cell >> 6, cell & 63, G >> 5
        rp, cb = w // wpr, w % wpr
        return (2 * rp + (lane >> 5)) * G + cb * 32 + (lane & 31)

    for G in (16, 32, 48, 64, 80, 96, 128, 160, 192, 240, 256, 320, 384, 40, 56):
        cells = np.array([remap(c, G) for c in range(G * G)])
        assert np.array_equal(np.sort(cells), np.arange(G * G)), G
        if G % 32 == 0:
            cols = 32
            for w0 in (0, 64 * 3, G * G - 64):
                blk = cells[w0:w0 + 64]
                r, c = blk // G, blk % G
                assert r.max() - r.min() == 64 // cols - 1 and c.max() - c.min() == cols - 1 and len(set(blk.tolist())) == 64, (G, w0)
        else:
            assert np.array_equal(cells, np.arange(G * G))
