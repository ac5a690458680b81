"""The bf16 training class of the refiner conv block (csrc/conv_stack_train_bf16.hip, ops.conv_block_train_bf16,
ConvRefiner.train_conv_impl = "hip_bf16") without a GPU: the host checks of the C entry points, the register budget of the kernels,
the refiner switch, and `reference_bf16_block` / `reference_bf16_chain` -- the float64 restatement of the block with bf16 rounding at
chosen points that tests/test_conv_train_bf16_gpu.py calibrates its bound with (test_conv_train_amp_cpu.py's, which hard-codes
`.half()`, with the rounding points unchanged).

The bound of both files, for every tensor T of a block (y, gx, seven parameter gradients, two running buffers):
    max|T_got - T64| <= max(2 * max|T_ref - T64|, 2^-8 * max(1, max|T64|))
T64: float64 on the rounded operands (x, dw_w, pw_w, gy rounded to bf16) with no rounding inside ("exact"); T_ref: the modules' own
class under torch.autocast(dtype=bfloat16), bf16 at every module output, every module's grad-input and the parameter gradients
("autocast"); all three with the same ReLU mask.  2^-8 is bf16's half-ulp at 1, as 2^-11 is fp16's in test_conv_train_amp_cpu.py,
whose docstring gives the reason for the factor 2.

ReLU mask band: a pre-ReLU value within a bf16 ulp of zero may flip a mask bit; the band |pre64| <= 2^-7 (1 + |u64|) |alpha64| is
test_conv_train_amp_gpu.py's 2^-10 scaled by the ulp ratio of the two formats, and it may hold at most 1.5 % of a case's cells -- a
condition on the inputs (measured on the CPU: 0.57 % .. 0.90 %), not a tolerance."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_conv_train_cpu import assert_train_kernels_have_no_spills_and_no_scratch
from test_conv_train_gpu import CASES, EPS, LEAVES, MOMENTUM, make_inputs

PARAMS = LEAVES[1:]
HALF_ULP = 2.0 ** -8        # bf16's half-ulp at 1
MASK_BAND = 2.0 ** -7       # |pre64| <= MASK_BAND (1 + |u64|) |alpha64|: where the device's mask may differ from float64's
MASK_BAND_SHARE = 0.015     # at most this share of a case's cells lies in the band


def to_bf16(x):
    """to the nearest bf16 value, kept in float64"""
    return x.float().bfloat16().double()


class _RoundBF16(torch.autograd.Function):
    """Straight-through rounding to the nearest bf16 value, kept in float64: of the value (fw), of its gradient (bw), or both."""

    @staticmethod
    def forward(ctx, x, fw, bw):
        ctx.bw = bw
        return to_bf16(x) if fw else x

    @staticmethod
    def backward(ctx, g):
        return (to_bf16(g) if ctx.bw else g), None, None


def rbf(x, fw=True, bw=True):
    return _RoundBF16.apply(x, fw, bw)


MODES = ("exact", "autocast", "hip")


def reference_bf16_chain(blocks, x, gy, masks=None, mode="autocast", momentum=MOMENTUM):
    """float64 on the CPU: len(blocks) conv blocks in a row, block i with the parameters of the make_inputs dict blocks[i], the first
    reading the fp32 map x, and the gradients of sum(y * bf16(gy)).  mode places the bf16 roundings:
      "exact"     the operands only: x, the depthwise taps, the 1x1 weights (and gy)
      "autocast"  torch.autocast(dtype=bfloat16) around the modules: every module output (u, relu(bn(u)), y) and the gradient that
                  enters it, conv weights and biases as operands and their gradients (cast back from a bf16 copy), the gradient
                  of x (the backward of its cast)
      "hip"       this package's class: u, t = relu(bn(u)) and y forward, gz (the gradient of t) and the gradient of a bf16 input
                  map backward; biases, the first block's gx and all parameter gradients stay fp32
    masks: per block a fixed 0/1 ReLU mask instead of pre > 0.  Returns y, per block pre / u / alpha / mask / rm / rv, and grads
    {"x": ..., (block, name): ...}."""
    assert mode in MODES
    ac, hip = mode == "autocast", mode == "hip"
    leaves = [{k: b[k].double().requires_grad_() for k in PARAMS if b[k] is not None} for b in blocks]
    x = x.double().requires_grad_()
    out = {"pre": [], "u": [], "alpha": [], "mask": [], "rm": [], "rv": []}
    h = x
    for i, (b, t) in enumerate(zip(blocks, leaves)):
        C = h.shape[1]
        if mode == "exact":
            xin = rbf(h, True, False) if i == 0 else h
        else:
            xin = rbf(h, True, ac or i > 0)
        dw_w, pw_w = rbf(t["dw_w"], True, ac), rbf(t["pw_w"], True, ac)
        dw_b, pw_b = t.get("dw_b"), t["pw_b"]
        if ac:
            dw_b, pw_b = (rbf(dw_b) if dw_b is not None else None), rbf(pw_b)
        u = F.conv2d(xin, dw_w, dw_b, padding=2, groups=C)
        if ac or hip:
            u = rbf(u, True, ac)
        rm, rv = b["rm"].double().clone(), b["rv"].double().clone()
        pre = F.batch_norm(u, rm, rv, t["bn_w"], t["bn_b"], training=True, momentum=momentum, eps=EPS)
        mask = (pre.detach() > 0).double() if masks is None else masks[i].double()
        tt = pre * mask
        if ac or hip:
            tt = rbf(tt, True, True)
        h = F.conv2d(tt, pw_w, pw_b)
        if ac or hip:
            h = rbf(h, True, True)
        var = u.detach().var(dim=(0, 2, 3), unbiased=False)
        for k, v in (("pre", pre.detach()), ("u", u.detach()), ("alpha", (t["bn_w"].detach() / torch.sqrt(var + EPS)).view(1, -1, 1, 1)),
                     ("mask", mask), ("rm", rm), ("rv", rv)):
            out[k].append(v)
    keys = [(i, k) for i, t in enumerate(leaves) for k in t]
    grads = torch.autograd.grad(h, [x] + [leaves[i][k] for i, k in keys], to_bf16(gy))
    out["y"] = h.detach()
    out["grads"] = dict(zip(["x"] + keys, grads))
    return out


def reference_bf16_block(inp, mask=None, mode="autocast", momentum=MOMENTUM):
    """One block of reference_bf16_chain on a make_inputs dict: {"y", "rm", "rv", "pre", "u", "alpha", "mask", "grads": {leaf: ...}}"""
    r = reference_bf16_chain([inp], inp["x"], inp["gy"], None if mask is None else [mask], mode, momentum)
    one = {k: r[k][0] for k in ("pre", "u", "alpha", "mask", "rm", "rv")}
    one["y"] = r["y"]
    one["grads"] = {"x": r["grads"]["x"], **{k: r["grads"][(0, k)] for k in PARAMS if (0, k) in r["grads"]}}
    return one


def bound_ratio(got, ref, exact):
    """max|got - exact| over the bound max(2 max|ref - exact|, 2^-8 max(1, max|exact|))"""
    err, cal = float((got.double() - exact).abs().max()), float((ref.double() - exact).abs().max())
    return err / max(2.0 * cal, HALF_ULP * max(1.0, float(exact.abs().max())))


def block_ratios(got, ref, exact):
    """bound_ratio per tensor kind of a block: y, the running buffers, every gradient the block has"""
    ratios = {k: bound_ratio(got[k], ref[k], exact[k]) for k in ("y", "rm", "rv")}
    for k, want in exact["grads"].items():
        ratios["d" + k] = bound_ratio(got["grads"][k], ref["grads"][k], want)
    return ratios


def mask_band(true64):
    """the cells of a float64 block whose pre-ReLU value lies within a bf16 ulp of zero"""
    return true64["pre"].abs() <= MASK_BAND * (1 + true64["u"].abs()) * true64["alpha"].abs()


def is_bf16_valued(t):
    return torch.equal(t.float().bfloat16().to(t.dtype), t)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------
def test_bf16_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every call below has exactly one bad argument and must be refused by the host checks, before a launch (every pointer is a
    host buffer that no kernel may ever see; the workspace it claims is large enough, so only the argument under test can refuse)."""
    from gfnet_amd import _lib

    assert _lib.BF16 == _lib.GFN_BF16 == 2 and _lib.GFN_F32 == 0 and _lib.GFN_F16 == 1
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    q, r = ctypes.c_void_p(p.value + 16), ctypes.c_void_p(p.value + 32)   # x, u and y must differ
    BIG = 1 << 40

    def fwd(x=p, x_dtype=_lib.GFN_F32, dw_w=p, dw_b=p, bn_w=p, bn_b=p, rm=p, rv=p, pw_w=p, pw_b=p, u=q, mean=p, invstd=p, y=r, B=2, C=24,
            M=24, G=16, momentum=0.1, eps=1e-5, ws=p, nws=BIG):
        return L.gfn_conv_block_train_bf16_fwd(x, x_dtype, dw_w, dw_b, bn_w, bn_b, rm, rv, pw_w, pw_b, u, mean, invstd, y, B, C, M, G, momentum,
                                               eps, ws, nws, None)

    def bwd(gy=p, x=p, x_dtype=_lib.GFN_BF16, u=p, mean=p, invstd=p, dw_w=p, bn_w=p, bn_b=p, pw_w=p, gx=p, d_dw_w=p, d_dw_b=p, d_bn_w=p,
            d_bn_b=p, d_pw_w=p, d_pw_b=p, B=2, C=24, M=24, G=16, need=15, ws=p, nws=BIG):
        return L.gfn_conv_block_train_bf16_bwd(gy, x, x_dtype, u, mean, invstd, dw_w, bn_w, bn_b, pw_w, gx, d_dw_w, d_dw_b, d_bn_w, d_bn_b,
                                               d_pw_w, d_pw_b, B, C, M, G, need, ws, nws, None)

    def refused(code, what, scratch=False):
        assert code == (-3 if scratch else -1), what
        assert L.gfn_last_error(), what

    need_fwd = int(L.gfn_conv_block_train_bf16_ws_bytes(2, 24, 24, 16, 0))
    need_bwd = int(L.gfn_conv_block_train_bf16_ws_bytes(2, 24, 24, 16, 1))
    assert need_fwd == 24 * 2 * 1 * 2 * 4                  # one 32x32 tile per 16x16 map, (mean, M2) per tile and channel
    assert need_bwd == int(L.gfn_conv_block_train_half_ws_bytes(2, 24, 24, 16, 1))      # the fp16 class's plan: a 2-byte gz map
    assert need_bwd < int(L.gfn_conv_block_train_ws_bytes(2, 24, 24, 16, 1))
    assert L.gfn_conv_block_train_bf16_ws_bytes(0, 24, 24, 16, 1) == 0 and L.gfn_conv_block_train_bf16_ws_bytes(2, 0, 24, 16, 0) == 0

    for name in ("x", "dw_w", "bn_w", "bn_b", "rm", "rv", "pw_w", "pw_b", "u", "mean", "invstd", "y"):
        refused(fwd(**{name: None}), f"fwd: null {name}")
    for what, kw in {"x_dtype = GFN_F16": dict(x_dtype=_lib.GFN_F16), "x_dtype = 7": dict(x_dtype=7), "x_dtype < 0": dict(x_dtype=-1),
                     "C = 0": dict(C=0), "M = 0": dict(M=0), "G = 0": dict(G=0), "B < 0": dict(B=-1),
                     "a map of 2^29 values": dict(C=1 << 13, G=1 << 8), "batch > 65535": dict(B=65536),
                     "too many row tiles": dict(C=65535 * 32 + 1, G=2), "u aliases x": dict(u=p), "y aliases u": dict(y=q),
                     "y aliases x": dict(y=p), "one value per channel": dict(B=1, G=1), "momentum > 1": dict(momentum=1.5),
                     "momentum < 0": dict(momentum=-0.1), "negative eps": dict(eps=-1.0)}.items():
        refused(fwd(**kw), "fwd: " + what)
    for what, kw in {"null workspace": dict(ws=None), "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 4)),
                     "workspace too small": dict(nws=need_fwd - 1)}.items():
        refused(fwd(**kw), "fwd: " + what, scratch=True)
    assert fwd(B=0) == 0 and fwd(B=0, x_dtype=_lib.GFN_BF16) == 0     # nothing to compute: valid, and no launch

    for name in ("gy", "x", "u", "mean", "invstd", "dw_w", "bn_w", "bn_b", "pw_w"):
        refused(bwd(**{name: None}), f"bwd: null {name}")
    for what, kw in {"x_dtype = GFN_F16": dict(x_dtype=_lib.GFN_F16), "x_dtype = 7": dict(x_dtype=7), "C = 0": dict(C=0), "M < 0": dict(M=-1),
                     "G = 0": dict(G=0), "B < 0": dict(B=-1), "a map of 2^29 values": dict(M=1 << 13, G=1 << 8),
                     "batch > 65535": dict(B=65536), "too many row tiles": dict(M=65535 * 32 + 1, G=2),
                     "one value per channel": dict(B=1, G=1), "need = 16": dict(need=16), "need < 0": dict(need=-1),
                     "need x without gx": dict(gx=None), "need dw without d_dw_w": dict(d_dw_w=None),
                     "need bn without d_bn_w": dict(d_bn_w=None), "need bn without d_bn_b": dict(d_bn_b=None),
                     "need pw without d_pw_w": dict(d_pw_w=None), "need pw without d_pw_b": dict(d_pw_b=None)}.items():
        refused(bwd(**kw), "bwd: " + what)
    for what, kw in {"null workspace": dict(ws=None), "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 8)),
                     "workspace too small": dict(nws=need_bwd - 1)}.items():
        refused(bwd(**kw), "bwd: " + what, scratch=True)
    assert bwd(B=0) == 0 and bwd(need=0) == 0 and bwd(need=0, d_dw_b=None, gx=None, x_dtype=_lib.GFN_F32) == 0
    # the fp16 class's entry points keep refusing bf16
    assert L.gfn_conv_block_train_half_fwd(p, _lib.GFN_BF16, p, p, p, p, p, p, p, p, q, p, p, r, 2, 24, 24, 16, 0.1, 1e-5, p, BIG, None) == -1


def test_bf16_kernels_have_no_spills_and_no_scratch():
    # the fp16 object's inventory, instantiated over the other element: 4 small reductions + the depthwise forward and backward for
    # fp32 / bf16 x + the 1x1 forward and backward + 8 shapes of the 1x1 weight gradient
    assert_train_kernels_have_no_spills_and_no_scratch("conv_stack_train_bf16.o", 4 + 2 + 2 + 1 + 1 + 8)


def test_hip_bf16_is_accepted_and_leaves_the_other_predicates_alone():
    from gfnet_amd.model.network import ConvRefiner

    ref = ConvRefiner(24, 24, 3, dw=True, hidden_blocks=2, displacement_emb="linear", displacement_emb_dim=8, local_corr_num=0,
                      corr_in_other=False, amp=True, amp_dtype=torch.bfloat16)
    assert ref.train_conv_impl == "torch" and ref.amp_dtype is torch.bfloat16
    ref.train_conv_impl = "hip_bf16"
    ref.train()
    d = torch.zeros(1, 24, 8, 8)
    assert not ref._hip_stack_supported() and not ref._hip_train_stack_supported(d) and not ref._hip_amp_train_stack_supported(d)
    assert not ref._hip_bf16_train_stack_supported(d)             # a CPU map: the modules
    ref.eval()
    assert ref._hip_stack_supported() and not ref._hip_bf16_train_stack_supported(d)
    ref.train()
    for impl in ("hip", "hip_amp", "torch"):
        ref.train_conv_impl = impl
        assert not ref._hip_bf16_train_stack_supported(d) and not ref._hip_amp_train_stack_supported(d)
    # everything but the device holds: the predicate follows the switch, amp and amp_dtype
    ref.train_conv_impl = "hip_bf16"
    ref._train_blocks_supported = lambda d: True
    assert ref._hip_bf16_train_stack_supported(d)
    ref.amp_dtype = torch.float16
    assert not ref._hip_bf16_train_stack_supported(d) and not ref._hip_amp_train_stack_supported(d)
    ref.amp_dtype, ref.amp = torch.bfloat16, False
    assert not ref._hip_bf16_train_stack_supported(d)
    ref.amp, ref.train_conv_impl = True, "hip_amp"
    assert not ref._hip_bf16_train_stack_supported(d) and not ref._hip_amp_train_stack_supported(d)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_cpu_autocast_rounds_where_the_restatement_says():
    """torch.autocast("cpu", dtype=torch.bfloat16) runs the block's modules and hands back bf16 at every module output; parameter
    gradients come back fp32 but bf16-valued (the cast of the bf16 copy's gradient), and so does the gradient of x."""
    inp = make_inputs(*CASES["narrow"])
    t = {k: inp[k].clone().requires_grad_() for k in LEAVES}
    C = inp["x"].shape[1]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        u = F.conv2d(t["x"], t["dw_w"], t["dw_b"], padding=2, groups=C)
        pre = F.batch_norm(u, None, None, t["bn_w"], t["bn_b"], training=True, eps=EPS)
        act = F.relu(pre)
        y = F.conv2d(act, t["pw_w"], t["pw_b"])
    assert u.dtype == pre.dtype == act.dtype == y.dtype == torch.bfloat16
    y.backward(inp["gy"].bfloat16())
    for k in LEAVES:
        assert t[k].grad.dtype == torch.float32, k
    for k in ("x", "dw_w", "dw_b", "pw_w", "pw_b"):
        assert is_bf16_valued(t[k].grad), f"d{k} did not pass through a bf16 tensor"


def test_restatement_rounds_at_its_points_and_takes_a_fixed_mask():
    inp = make_inputs(*CASES["g_not_4k_batch3"])
    ac, hip, exact = (reference_bf16_block(inp, mode=m) for m in ("autocast", "hip", "exact"))
    # the straight-through function: value and gradient each rounded on request, identity otherwise
    v = torch.tensor([1.0 + 2.0 ** -9, 70000.0, 1.0 + 3 * 2.0 ** -8, float("inf")], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([3.0 + 2.0 ** -8, 1.0, 1.0, 1.0], dtype=torch.float64)
    out = rbf(v)
    assert out.dtype == torch.float64 and out[0] == 1.0 and out[1] == 70144.0     # to nearest; past fp16's 65504 still finite
    assert out[2] == 1.0 + 2.0 ** -6 and torch.isinf(out[3])                      # a tie goes to the even neighbour; inf stays inf
    assert torch.isnan(rbf(torch.tensor([float("nan")], dtype=torch.float64))).all()
    assert torch.autograd.grad(out, v, g)[0][0] == 3.0
    assert torch.equal(torch.autograd.grad(rbf(v, True, False), v, g)[0], g) and torch.equal(rbf(v, False, True), v)
    for r in (ac, hip):
        assert r["y"].dtype == torch.float64 and is_bf16_valued(r["y"]) and is_bf16_valued(r["u"])
    assert not is_bf16_valued(exact["y"]) and not is_bf16_valued(exact["u"])
    for k in ("x", "dw_w", "dw_b", "pw_w", "pw_b"):
        assert is_bf16_valued(ac["grads"][k]), f"autocast d{k}"
    for k in ("x", "dw_w", "pw_w", "pw_b", "bn_w", "bn_b"):
        assert not is_bf16_valued(hip["grads"][k]), f"hip d{k}: the first block's gx and the parameter gradients stay fp32"
    # a chain's second block hands a bf16-valued gradient to the first block's y in both classes
    two = [inp, make_inputs(3, 37, 10, True, 5)]
    for mode in ("autocast", "hip"):
        h = inp["x"].double()
        r = reference_bf16_chain(two, inp["x"], inp["gy"], mode=mode)
        assert len(r["pre"]) == 2 and is_bf16_valued(r["y"]) and (1, "pw_w") in r["grads"] and h.shape == r["grads"]["x"].shape
    # a fixed mask replaces pre > 0: all closed, y is the rounded 1x1 bias and nothing but that bias has a gradient
    shut = reference_bf16_block(inp, mask=torch.zeros_like(inp["x"]), mode="hip")
    assert torch.equal(shut["y"], to_bf16(inp["pw_b"].double().view(1, -1, 1, 1).expand_as(shut["y"])))
    assert not shut["grads"]["x"].any() and not shut["grads"]["pw_w"].any() and shut["grads"]["pw_b"].any()
    assert torch.equal(reference_bf16_block(inp, mask=hip["mask"], mode="hip")["y"], hip["y"])


@pytest.mark.parametrize("name", list(CASES))
def test_the_bound_is_feasible_for_this_class(name):
    """The restatement with this class's rounding points stays inside the bound that the GPU test sets for the kernels, on all
    eight cases, with the float64 mask throughout (measured here: worst ratio 0.55, below_a_tile dbn_w)."""
    inp = make_inputs(*CASES[name])
    exact = reference_bf16_block(inp, mode="exact")
    ref, hip = (reference_bf16_block(inp, mask=exact["mask"], mode=m) for m in ("autocast", "hip"))
    ratios = block_ratios(hip, ref, exact)
    print(f"{name}: " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", list(CASES))
def test_the_mask_band_holds_few_cells(name):
    """A condition on the inputs: at most 1.5 % of a case's cells have a float64 pre-ReLU value within a bf16 ulp of zero, so a
    device mask that differs from float64's only there moves few cells."""
    true64 = reference_bf16_block(make_inputs(*CASES[name]), mode="exact")
    share = float(mask_band(true64).double().mean())
    print(f"{name}: band share {share:.5f}")
    assert share <= MASK_BAND_SHARE
