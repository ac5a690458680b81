"""Host side of the refiner-input backward (gfn_refiner_input_bwd): the two entry points are exported with the signatures
include/gfnet_hip.h declares, argument errors come back as codes before anything touches a device, ops.refiner_input has no CPU
path and refuses symmetric batches that need gradients, and ConvRefiner.assemble sends each sample mode the right way.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "gfn_stream_t": ctypes.c_void_p}


def declared_argtypes(name):
    """(return type, ctypes argument types) of `name` as include/gfnet_hip.h declares it; every pointer is a c_void_p"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gfnet_hip.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]])
    return m.group(1), args


def test_both_symbols_are_exported_with_the_declared_signatures():
    from gfnet_amd import _lib

    L = _lib.lib()
    ret, args = declared_argtypes("gfn_refiner_input_bwd")
    assert ret == "int" and len(args) == 23
    assert L.gfn_refiner_input_bwd.argtypes == args and L.gfn_refiner_input_bwd.restype == ctypes.c_int
    ret, args = declared_argtypes("gfn_refiner_input_bwd_scratch_bytes")
    assert ret == "int64_t" and args == [ctypes.c_int] * 3
    assert L.gfn_refiner_input_bwd_scratch_bytes.argtypes == args and L.gfn_refiner_input_bwd_scratch_bytes.restype == ctypes.c_int64


def test_scratch_bytes_is_positive_and_monotone():
    from gfnet_amd import _lib

    f = _lib.lib().gfn_refiner_input_bwd_scratch_bytes
    sizes = [(1, 1, 1), (1, 16, 1), (1, 17, 1), (1, 17, 8), (3, 17, 8), (3, 64, 8), (8, 256, 8), (8, 256, 64), (32, 320, 64)]
    got = [int(f(*s)) for s in sizes]
    assert all(v > 0 and v % 4 == 0 for v in got)
    assert got == sorted(got)
    assert got[0] == 3 * 4  # one workgroup, one embedding channel: three partial sums
    for B, G, Dd in sizes:  # monotone in each argument on its own
        assert f(B + 1, G, Dd) >= f(B, G, Dd) and f(B, G + 1, Dd) >= f(B, G, Dd) and f(B, G, Dd + 1) > f(B, G, Dd)


def test_argument_errors_are_codes_and_launch_nothing():
    from gfnet_amd import _lib

    L = _lib.lib()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below is refused first
    nul = ctypes.c_void_p(0)

    def call(grad_d=p, d_bs=10 ** 9, f1=p, dtype=0, flow=p, w=p, B=1, C=4, Hs=8, Ws=8, G=8, Dd=4, K=9, ddw=nul, scratch=nul, nscr=0):
        return L.gfn_refiner_input_bwd(grad_d, d_bs, f1, dtype, flow, w, nul, p, p, p, ddw, nul, B, C, Hs, Ws, G, Dd, K, 1.25, scratch, nscr, nul)

    assert call(dtype=2) == -1 and b"dtype" in L.gfn_last_error()
    for kw in (dict(grad_d=nul), dict(f1=nul), dict(flow=nul), dict(w=nul)):
        assert call(**kw) == -1 and b"null pointer" in L.gfn_last_error(), kw
    for kw in (dict(B=-1), dict(C=0), dict(Hs=0), dict(Ws=0), dict(G=0), dict(Dd=-1), dict(K=-1), dict(d_bs=(2 * 4 + 4 + 9) * 64 - 1),
               dict(Hs=1 << 16, Ws=1 << 15, C=1)):  # Hs * Ws = 2^31: pixel offsets are 32-bit
        assert call(**kw) == -1 and b"bad size" in L.gfn_last_error(), kw
    assert call(B=65536) == -1
    need = int(L.gfn_refiner_input_bwd_scratch_bytes(1, 8, 4))
    assert call(ddw=p) == -3 and call(ddw=p, scratch=p, nscr=need - 1) == -3 and b"scratch" in L.gfn_last_error()
    assert call(B=0) == 0  # an empty batch is nothing to do


def _tensors(B=2, flow_batch=None, C=4, hs=8, G=6, Dd=3, grad=("flow",)):
    t = dict(x=torch.randn(B, C, hs, hs), y=torch.randn(B, C, hs, hs), flow=torch.zeros(flow_batch or B, 2, G, G),
             w=torch.randn(Dd, 2, 1, 1), b=torch.randn(Dd))
    for k in grad:
        t[k].requires_grad_(True)
    return G, t


@pytest.mark.parametrize("who", ["x", "y", "flow", "w", "b"])
def test_cpu_tensors_raise_with_and_without_grad(who):
    from gfnet_amd import _lib, ops

    G, t = _tensors(grad=(who,))
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], 1)
    with torch.no_grad(), pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], 1)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.refiner_input_bwd(torch.zeros(2, 2 * 4 + 3 + 9, G, G), t["y"], t["flow"].detach(), t["w"].detach(), 1)


@pytest.mark.parametrize("who", ["x", "flow", "b"])
def test_symmetric_batch_with_grad_is_refused(who):
    from gfnet_amd import _lib, ops

    G, t = _tensors(flow_batch=4, grad=(who,))
    with pytest.raises(NotImplementedError, match="plain batch"):
        ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], 1)
    with torch.no_grad(), pytest.raises(_lib.GfnError, match="no CPU path"):  # without grad it is the inference launch
        ops.refiner_input(G, t["x"], t["y"], t["flow"], t["w"], t["b"], 1)


def _refiner(sample_mode):
    from gfnet_amd.model.network import ConvRefiner

    dim = 2 * 4 + 3 + 9
    return ConvRefiner(dim, dim, 3, kernel_size=5, dw=True, hidden_blocks=1, displacement_emb="linear", displacement_emb_dim=3,
                       local_corr_num=1, corr_in_other=True, amp=True, bn_momentum=0.01, sample_mode=sample_mode).train()


@pytest.mark.parametrize("sample_mode", ["bilinear", "nearest", "bicubic"])
@pytest.mark.parametrize("who", ["x", "y", "flow", "weight", "bias", None])
def test_assemble_routes_by_sample_mode_and_by_who_needs_a_gradient(monkeypatch, sample_mode, who):
    """bilinear: always ops.refiner_input (differentiable on its own); nearest / bicubic: _assemble_autograd as soon as anything
    that reaches d asks for a gradient -- the flow and disp_emb.bias included -- and the raw launch otherwise"""
    from gfnet_amd import ops

    ref = _refiner(sample_mode)
    for p in ref.parameters():
        p.requires_grad_(False)
    G, t = _tensors(grad=(who,) if who in ("x", "y", "flow") else ())
    if who in ("weight", "bias"):
        getattr(ref.disp_emb, who).requires_grad_(True)
    calls = []
    monkeypatch.setattr(ref, "_assemble_autograd", lambda *a: calls.append("torch") or ("d", "lc"))

    def launch(num_grid, x, y, flow, w, b, r, **kw):
        calls.append("hip")
        assert kw["reuse"] is None and kw["sample_mode"] == sample_mode and w is ref.disp_emb.weight and b is ref.disp_emb.bias
        return torch.zeros(2, 2 * 4 + 3 + 9, G, G)

    monkeypatch.setattr(ops, "refiner_input", launch)
    ref.assemble(G, t["x"], t["y"], t["flow"])
    assert calls == (["torch"] if sample_mode != "bilinear" and who is not None else ["hip"])
    calls.clear()
    with torch.no_grad():
        ref.assemble(G, t["x"], t["y"], t["flow"])
    assert calls == ["hip"]
