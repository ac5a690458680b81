"""ops.decoder_qkv and ops.decoder_post (csrc/decoder_block.hip) and CrossViewDecoder's block_impl="hip" on the GPU.

Oracle: the definition in float64 on the CPU, in plain torch, with no rounding anywhere (`definition_*` below on .double() inputs).

Unit: e16 = the error of the SAME sub-expression run by torch on the CPU under torch.autocast("cpu", dtype=torch.float16) against
that float64 result, computed here per case and per tensor, never fixed.  Bound: 4 * e16, the bound the existing autocast decoder
test (test_cross_attn_gpu.py) uses: the kernels round operands where the reference's autocast rounds the input of a Linear and keep
the Linear outputs fp32 where the reference rounds them too, so they sit inside the reference class.  Every comparison asserts
e16 > 0, so a degenerate unit cannot pass silently.

Each comparison also prints (without asserting) the kernel's error against a float64 emulation of its own arithmetic class: fp16
rounding of the weights, of the LayerNorm outputs, of the raw K and V rows, of the attention output and of the GELU output, and
nowhere else (q, k and v rounded once on the way out).

Measured on an MI355X, worst err / (4 e16) over all cases: q 0.44 ((2, 1) mean50: 1.6e-03 against e16 8.9e-04), k 0.25, v 0.25,
X_out 0.20 ((2, 30) large), the module's maps 0.16 / 0.18.  Against its own class: q, k, v within one fp16 ulp of the result, X_out
9.6e-04 at worst on values up to 9.
"""
import functools
import json
import os
import types

import numpy as np
import pytest
import synth
import torch
import torch.nn.functional as F

from gfnet_amd import ops
from gfnet_amd.model.crossview_decoder import CrossViewDecoder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g14_crossview_decoder.npz")
DEV = "cuda"
C, HID, EPS = 64, 256, 1e-5

# (2B, N): one row per view; the golden's shape; 74 rows, a tail in every tile size; several batch entries and tiles; 67,584 rows =
# 2112 tiles of 32, more than a persistent grid has waves for
SMALL = [(2, 1), (2, 30), (2, 37), (6, 100)]
BIG = (66, 1024)
FAMILIES = ("normal", "mean50", "constant", "large")
CASES = [(s, f) for s in SMALL for f in FAMILIES] + [(BIG, "normal")]


@functools.lru_cache(maxsize=None)
def params():
    """The parameters of one block as fp32 CPU tensors: weights 0.87 / sqrt(fan_in) times a unit lattice normal, LayerNorm weights
    around 1, gammas in [0.5, 1.5] (not the module's 1e-5: a dropped LayerScale must show)."""
    def n(shape, seed, scale=1.0):
        return torch.from_numpy(np.float32(scale / 1.15) * synth.lattice_normalish(shape, seed))

    def u(shape, seed):
        return torch.from_numpy(synth.lattice_uniform(shape, seed))

    p = types.SimpleNamespace(
        nw1=1 + 0.25 * u((C,), 11), nb1=0.25 * u((C,), 12), wq=n((C, C), 13, 0.87 / 8), wk=n((C, C), 14, 0.87 / 8), wv=n((C, C), 15, 0.87 / 8),
        wproj=n((C, C), 16, 0.87 / 8), bproj=0.25 * u((C,), 17), g1=1 + 0.5 * u((C,), 18), nw2=1 + 0.25 * u((C,), 19), nb2=0.25 * u((C,), 20),
        w1=n((HID, C), 21, 0.87 / 8), b1=0.25 * u((HID,), 22), w2=n((C, HID), 23, 0.87 / 16), b2=0.25 * u((C,), 24), g2=1 + 0.5 * u((C,), 25))
    assert float(p.g1.min()) >= 0.5 and float(p.g2.max()) <= 1.5
    return p


def cast(p, fn):
    return types.SimpleNamespace(**{k: fn(v) for k, v in vars(p).items()})


@functools.lru_cache(maxsize=None)
def rows(shape, family):
    """(X fp32 (2B, N, 64), attn fp16 (2B, N, 8, 8)) on the CPU."""
    B2, N = shape
    seed = (B2 * 4099 + N) * 7 + FAMILIES.index(family)
    X = torch.from_numpy(synth.lattice_normalish((B2, N, C), seed))
    attn = torch.from_numpy(synth.lattice_normalish((B2, N, 8, 8), seed + 500)).half()
    if family == "mean50":  # a one-pass variance, E[x^2] - mean^2, loses every digit of these rows' spread
        X = 50 + 1e-2 * X
    elif family == "constant":  # the variance is exactly 0; the post kernel's x1 stays constant with a zero attention row and bproj = 0
        X = (4 * X[..., :1]).expand(B2, N, C).contiguous()
        attn = torch.zeros_like(attn)
    elif family == "large":  # q, k and v toward the top of the fp16 range
        X = 1e3 * X
    return X, attn


def block_params(family):
    p = params()
    if family == "constant":
        p = types.SimpleNamespace(**{**vars(p), "bproj": torch.zeros(C)})
    return p


def definition_qkv(X, p):
    """block.py:327's norm1 and attention.py:236-238 in X's dtype; k and v NOT yet moved to the other view's batch entry."""
    return F.linear(F.layer_norm(X, (C,), p.nw1, p.nb1, EPS), p.wq), F.linear(X, p.wk), F.linear(X, p.wv)


def definition_post(X, attn, p):
    """attention.py:255 and the rest of block.py:327-328 (layer_scale.py, mlp.py) in X's dtype."""
    x1 = X + p.g1 * F.linear(attn.reshape(X.shape), p.wproj, p.bproj)
    return x1 + p.g2 * F.linear(F.gelu(F.linear(F.layer_norm(x1, (C,), p.nw2, p.nb2, EPS), p.w1, p.b1)), p.w2, p.b2)


def r16(t):
    return t.half().double()


def class_qkv(X, p):
    """The kernel's arithmetic class in float64: fp16 weights, fp16 LayerNorm output and raw rows, results rounded once."""
    X = X.double()
    n = F.layer_norm(X, (C,), p.nw1.double(), p.nb1.double(), EPS)
    return tuple(r16(F.linear(r16(a), r16(w))) for a, w in ((n, p.wq), (X, p.wk), (X, p.wv)))


def class_post(X, attn, p):
    d = cast(p, lambda t: t.double())
    X = X.double()
    x1 = X + d.g1 * F.linear(attn.double().reshape(X.shape), r16(p.wproj), d.bproj)
    h = r16(F.layer_norm(x1, (C,), d.nw2, d.nb2, EPS))
    return x1 + d.g2 * F.linear(r16(F.gelu(F.linear(h, r16(p.w1), d.b1))), r16(p.w2), d.b2)


@functools.lru_cache(maxsize=None)
def references(shape, family):
    """Per tensor (q, k, v, post): (float64 definition, e16, float64 emulation of the kernel's class); k and v where the kernel
    writes them.  Computed once per case and shared."""
    X, attn = rows(shape, family)
    p = block_params(family)
    p64 = cast(p, lambda t: t.double())
    B = shape[0] // 2
    with torch.no_grad():
        want = list(definition_qkv(X.double(), p64)) + [definition_post(X.double(), attn.double(), p64)]
        with torch.autocast(device_type="cpu", dtype=torch.float16):
            emu = list(definition_qkv(X, p)) + [definition_post(X, attn, p)]
        cls = list(class_qkv(X, p)) + [class_post(X, attn, p)]
    out = {}
    for i, name in enumerate(("q", "k", "v", "post")):
        w, e, c = want[i], emu[i].double(), cls[i]
        if name in "kv":
            w, e, c = (t.roll(B, 0) for t in (w, e, c))
        out[name] = (w, float((e - w).abs().max()), c)
    return out


def gpu(p):
    return cast(p, lambda t: t.to(DEV))


def run_qkv(X, p):
    return ops.decoder_qkv(X, p.nw1, p.nb1, EPS, p.wq, p.wk, p.wv)


def run_post(X, attn, p, inplace=False):
    return ops.decoder_post(X, attn, p.wproj, p.bproj, p.g1, p.nw2, p.nb2, EPS, p.w1, p.b1, p.w2, p.b2, p.g2, inplace=inplace)


def compare(what, got, ref):
    want, e16, cls = ref
    got = got.double().cpu().reshape(want.shape)
    err, ecls = float((got - want).abs().max()), float((got - cls).abs().max())
    print(f"{what}: err {err:.3e}  e16 {e16:.3e}  err / (4 e16) {err / (4 * e16) if e16 else float('inf'):.3f}  against its own class {ecls:.3e}"
          f"  max|ref| {float(want.abs().max()):.3e}")
    assert e16 > 0, what
    assert torch.isfinite(got).all() and err <= 4 * e16, (what, err, 4 * e16)


@pytest.mark.parametrize("shape,family", CASES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in CASES])
def test_qkv_against_the_float64_definition(shape, family):
    X, _ = rows(shape, family)
    ref = references(shape, family)
    with torch.no_grad():
        q, k, v = run_qkv(X.to(DEV), gpu(block_params(family)))
    assert q.dtype == k.dtype == v.dtype == torch.float16 and q.shape == k.shape == v.shape == (shape[0], shape[1], 8, 8)
    for name, t in zip("qkv", (q, k, v)):
        compare(f"decoder_qkv {shape} {family} {name}", t, ref[name])


@pytest.mark.parametrize("shape,family", CASES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in CASES])
def test_post_against_the_float64_definition(shape, family):
    X, attn = rows(shape, family)
    with torch.no_grad():
        out = run_post(X.to(DEV), attn.to(DEV), gpu(block_params(family)))
    assert out.dtype == torch.float32 and out.shape == X.shape
    compare(f"decoder_post {shape} {family}", out, references(shape, family)["post"])


def small_ints(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def test_qkv_k_and_v_are_exact_on_small_integers_and_land_on_the_other_view():
    """Small-integer rows and weights: every product and sum is exact (|sum| <= 64 * 4 * 2 < 2048), so k and v equal F.linear in
    fp16 bit for bit, at batch entry (b + B) mod 2B."""
    B2, N = 6, 37
    X = small_ints((B2, N, C), 1, -4, 4)
    p = types.SimpleNamespace(**{**vars(params()), "wk": small_ints((C, C), 2, -2, 2), "wv": small_ints((C, C), 3, -2, 2)})
    with torch.no_grad():
        _, k, v = run_qkv(X.to(DEV), gpu(p))
    for got, w in ((k, p.wk), (v, p.wv)):
        want = F.linear(X, w).half().reshape(B2, N, 8, 8)  # exact in fp32, exact in fp16
        assert float(want.float().abs().max()) > 50
        for b in range(B2):
            assert torch.equal(got[(b + B2 // 2) % B2].cpu(), want[b]), b


def test_post_is_exact_on_small_integers_with_the_mlp_scaled_to_zero():
    """gamma2 = 0 and small-integer a, wproj, bproj, gamma1 and x: X_out = x + gamma1 * (wproj . a + bproj) bit for bit."""
    rows_ = (6, 37, C)
    X, a = small_ints(rows_, 4, -8, 8), small_ints(rows_, 5, -3, 3).half()
    p = types.SimpleNamespace(**{**vars(params()), "wproj": small_ints((C, C), 6, -2, 2), "bproj": small_ints((C,), 7, -5, 5),
                                 "g1": small_ints((C,), 8, 1, 3), "g2": torch.zeros(C)})
    want = X + p.g1 * F.linear(a.float(), p.wproj, p.bproj)
    with torch.no_grad():
        got = run_post(X.to(DEV), a.to(DEV).reshape(6, 37, 8, 8), gpu(p))
    assert float((want - X).abs().max()) > 50 and torch.equal(got.cpu(), want)


def test_post_inplace_gives_the_same_bits_and_writes_over_x():
    X, attn = rows((2, 37), "normal")
    p = gpu(params())
    with torch.no_grad():
        out = run_post(X.to(DEV), attn.to(DEV), p)
        Xd = X.to(DEV)
        ret = run_post(Xd, attn.to(DEV), p, inplace=True)
    assert ret.data_ptr() == Xd.data_ptr() and torch.equal(Xd, out) and not torch.equal(Xd.cpu(), X)


def unswap(t):
    """k or v with every row back at the batch entry it was computed from."""
    return t.roll(-(t.shape[0] // 2), 0)


def test_a_rows_result_does_not_depend_on_its_position_or_on_the_call():
    """The first 74 rows of a 300-row call equal the 74-row call bit for bit, and two identical calls are bit-identical."""
    g = torch.Generator().manual_seed(9)
    X = torch.randn(300, C, generator=g).to(DEV)
    attn = torch.randn(300, C, generator=g).half().to(DEV)
    p = gpu(params())
    with torch.no_grad():
        big = [t.reshape(300, C) for t in run_qkv(X.reshape(2, 150, C), p)]
        again = [t.reshape(300, C) for t in run_qkv(X.reshape(2, 150, C), p)]
        small = [t.reshape(74, C) for t in run_qkv(X[:74].reshape(2, 37, C).contiguous(), p)]
        pbig, pagain = run_post(X, attn, p), run_post(X, attn, p)
        psmall = run_post(X[:74].contiguous(), attn[:74].contiguous(), p)
    for a, b in zip(big, again):
        assert torch.equal(a, b)
    assert torch.equal(big[0][:74], small[0])
    for i in (1, 2):
        assert torch.equal(unswap(big[i].reshape(2, 150, C)).reshape(300, C)[:74], unswap(small[i].reshape(2, 37, C)).reshape(74, C))
    assert torch.equal(pbig, pagain) and torch.equal(pbig[:74], psmall)


def test_a_non_finite_row_stays_in_its_row():
    """One row of inf and one of nan make only their own rows non-finite; every other row is bit-identical to a clean call."""
    X, attn = (t.clone() for t in rows((6, 100), "normal"))
    p = gpu(params())
    bad = [(1, 17), (4, 99)]
    Xb, ab = X.clone(), attn.clone()
    Xb[bad[0]], Xb[bad[1]] = float("inf"), float("nan")
    ab[bad[0]], ab[bad[1]] = float("nan"), float("inf")
    with torch.no_grad():
        clean = [unswap(t) if i else t for i, t in enumerate(run_qkv(X.to(DEV), p))] + [run_post(X.to(DEV), attn.to(DEV), p),
                                                                                         run_post(X.to(DEV), attn.to(DEV), p)]
        dirty = [unswap(t) if i else t for i, t in enumerate(run_qkv(Xb.to(DEV), p))] + [run_post(Xb.to(DEV), attn.to(DEV), p),
                                                                                          run_post(X.to(DEV), ab.to(DEV), p)]
    mask = torch.ones(6, 100, dtype=torch.bool)
    for b, n in bad:
        mask[b, n] = False
    for name, c, d in zip(("q", "k", "v", "post(x)", "post(attn)"), clean, dirty):
        c, d = c.cpu().reshape(6, 100, C), d.cpu().reshape(6, 100, C)
        assert torch.isfinite(c).all(), name
        assert torch.equal(c[mask], d[mask]), name
        assert not torch.isfinite(d[~mask]).any(), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_the_ops_refuse_what_the_kernels_are_not_built_for():
    X, attn = (t.to(DEV) for t in rows((2, 37), "normal"))
    p = gpu(params())
    with torch.no_grad():
        with pytest.raises(TypeError, match="attn"):
            run_post(X, attn.float(), p)
        with pytest.raises(TypeError, match="X"):
            run_qkv(X.half(), p)
        with pytest.raises(ValueError, match="X must be contiguous"):
            run_post(X.transpose(0, 1).contiguous().transpose(0, 1), attn, p)
        with pytest.raises(ValueError, match="X must be contiguous"):
            run_qkv(X.transpose(0, 1).contiguous().transpose(0, 1), p)
        with pytest.raises(ValueError, match="w1"):
            run_post(X, attn, types.SimpleNamespace(**{**vars(p), "w1": p.w1[:128].contiguous()}))
        with pytest.raises(ValueError, match="even batch"):
            run_qkv(X[:1], p)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="requires grad"):
            run_post(X.clone().requires_grad_(), attn, p)
        with pytest.raises(RuntimeError, match="wq requires grad"):
            run_qkv(X, types.SimpleNamespace(**{**vars(p), "wq": p.wq.clone().requires_grad_()}))
        run_qkv(X, p)  # grad mode alone is no reason


# ---- the module ----------------------------------------------------------------------------------------------------------------
def load_golden():
    z = np.load(GOLDEN)
    state = {k[len("param/"):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("param/")}
    x, y = (torch.from_numpy(z[k].astype(np.float32)) for k in ("x", "y"))
    return json.loads(str(z["conf"])), state, x, y, tuple(int(v) for v in z["grid"])


def decoder(attn_impl, block_impl, device="cpu", dtype=torch.float32):
    conf, state, *_ = load_golden()
    dec = CrossViewDecoder(conf, attn_impl=attn_impl, block_impl=block_impl)
    dec.load_state_dict(state, strict=True)
    return dec.train(False).to(device, dtype)


def test_module_with_fused_blocks_under_fp16_autocast():
    """block_impl="hip" on the g14 golden under CUDA fp16 autocast against the float64 module, within 4 x the error of the torch
    module on the CPU under fp16 autocast, per map; swapping the views swaps the maps bit for bit."""
    _, _, x, y, (B, H, W) = load_golden()
    shape = (B, 3, H, W)
    dec = decoder("hip", "hip", DEV)
    with torch.no_grad():
        want = decoder("torch", "torch", dtype=torch.float64)(x.double(), y.double(), vit_shape=shape)
        with torch.autocast(device_type="cpu", dtype=torch.float16):
            emu = decoder("torch", "torch")(x, y, vit_shape=shape)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            assert dec._fused(x.to(DEV), y.to(DEV))
            got = dec(x.to(DEV), y.to(DEV), vit_shape=shape)
            swapped = dec(y.to(DEV), x.to(DEV), vit_shape=shape)
    for name, a, e, b in zip("xy", got, emu, want):
        e16 = float((e.double() - b).abs().max())
        err = float((a.double().cpu() - b).abs().max())
        print(f"fused decoder map {name}: err {err:.3e}  e16 {e16:.3e}  err / (4 e16) {err / (4 * e16):.3f}  max|map| {float(b.abs().max()):.2f}")
        assert e16 > 0 and a.dtype == torch.float32 and a.shape == b.shape
        assert torch.isfinite(a).all() and err <= 4 * e16, (name, err, 4 * e16)
    assert torch.equal(swapped[0], got[1]) and torch.equal(swapped[1], got[0])


def test_module_without_layerscale_takes_a_gamma_of_one():
    """init_values None leaves nn.Identity where the LayerScales were: the fused path passes a gamma of 1.  Same oracle, unit and
    bound as above, on the golden's inputs with freshly initialised weights."""
    conf, _, x, y, (B, H, W) = load_golden()
    conf["dino_cfg"]["decoder_cfg"]["init_values"] = None
    shape = (B, 3, H, W)
    torch.manual_seed(3)
    dec = CrossViewDecoder(conf, attn_impl="hip", block_impl="hip").train(False)
    ref = CrossViewDecoder(conf, attn_impl="torch").train(False)
    ref.load_state_dict(dec.state_dict())
    assert not any("gamma" in k for k in dec.state_dict())
    with torch.no_grad():
        with torch.autocast(device_type="cpu", dtype=torch.float16):
            emu = ref(x, y, vit_shape=shape)
        want = ref.double()(x.double(), y.double(), vit_shape=shape)
        dec.to(DEV)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            assert dec._fused(x.to(DEV), y.to(DEV))
            got = dec(x.to(DEV), y.to(DEV), vit_shape=shape)
    for name, a, e, b in zip("xy", got, emu, want):
        e16 = float((e.double() - b).abs().max())
        err = float((a.double().cpu() - b).abs().max())
        print(f"fused decoder without LayerScale, map {name}: err {err:.3e}  e16 {e16:.3e}  err / (4 e16) {err / (4 * e16):.3f}")
        assert e16 > 0 and torch.isfinite(a).all() and err <= 4 * e16, (name, err, 4 * e16)


def test_module_outside_the_fused_class_is_the_torch_path_bit_for_bit():
    """fp32 without autocast, and train() under autocast: block_impl="hip" equals block_impl="torch" bit for bit."""
    _, _, x, y, (B, H, W) = load_golden()
    shape = (B, 3, H, W)
    hip, ref = decoder("hip", "hip", DEV), decoder("hip", "torch", DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        assert not hip._fused(xd, yd)
        for a, b in zip(hip(xd, yd, vit_shape=shape), ref(xd, yd, vit_shape=shape)):
            assert torch.equal(a, b)
    hip.train(), ref.train()
    with torch.autocast(device_type="cuda", dtype=torch.float16):
        assert not hip._fused(xd, yd)
        outs = hip(xd, yd, vit_shape=shape), ref(xd, yd, vit_shape=shape)
    for a, b in zip(*outs):
        assert a.requires_grad and torch.equal(a, b)
    hip.train(False)
    with torch.autocast(device_type="cuda", dtype=torch.float16):  # eval(), but grad mode on and parameters that require grad
        assert not hip._fused(xd, yd)


def test_a_fused_forward_is_three_launches_per_block():
    conf, _, x, y, (B, H, W) = load_golden()
    dec = decoder("hip", "hip", DEV)
    names = ("decoder_qkv", "cross_attn_fwd", "decoder_post")
    ops.kernel_events = {n: [] for n in names}
    try:
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.float16):
            dec(x.to(DEV), y.to(DEV), vit_shape=(B, 3, H, W))
        torch.cuda.synchronize()
        counts = {n: len(v) for n, v in ops.kernel_events.items()}
    finally:
        ops.kernel_events = None
    blocks = conf["dino_cfg"]["decoder_cfg"]["num_cross_attn"]
    assert blocks >= 1 and counts == {n: blocks for n in names}, counts
