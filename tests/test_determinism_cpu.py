"""Host side of the bit-reproducible training path: the workspace formula of gfn_refiner_input_bwd_det, the refusals of it and of
gfn_interp_bilinear_bwd before anything touches a device, how the `deterministic` keyword resolves against
torch.use_deterministic_algorithms, and that ops.resize_bilinear has no CPU path.  No GPU."""
import ctypes

import pytest
import torch


@pytest.fixture
def restore_flag():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def test_workspace_formula_is_monotone_a_multiple_of_eight_and_zero_when_empty():
    from gfnet_amd import _lib

    f = _lib.lib().gfn_refiner_input_bwd_det_ws_bytes
    for empty in ((0, 4, 8, 8), (2, 0, 8, 8), (2, 4, 0, 8), (2, 4, 8, 0), (-1, 4, 8, 8)):
        assert int(f(*empty)) == 0, empty
    sizes = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 7, 9), (1, 3, 12, 10), (2, 9, 8, 8), (3, 16, 64, 64), (8, 8, 448, 448), (32, 64, 512, 512)]
    got = [int(f(*s)) for s in sizes]
    assert all(v > 0 and v % 8 == 0 for v in got) and got == sorted(got)
    assert got[0] == 8 + 8 + 8  # one accumulator, one flag word and one sample word, each padded to 8 bytes
    for B, C, Hs, Ws in sizes:
        n = B * C * Hs * Ws
        assert int(f(B, C, Hs, Ws)) >= 8 * n + (n + 7) // 8 + 4 * B  # an accumulator and a bit per element, a word per sample
        for bigger in ((B + 1, C, Hs, Ws), (B, C + 1, Hs, Ws), (B, C, Hs + 1, Ws), (B, C, Hs, Ws + 1)):
            assert f(*bigger) > f(B, C, Hs, Ws)
    assert int(f(65535, 8, 16384, 16384)) == 8 * 65535 * 8 * 2 ** 28 + 65535 * 2 ** 28 + 65536 * 4  # 64-bit arithmetic


def test_det_entry_point_refuses_on_the_host():
    from gfnet_amd import _lib

    L = _lib.lib()
    p, odd, nul = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(0)  # never dereferenced: every call below is refused first

    def call(grad_d=p, d_bs=10 ** 9, f1=p, dtype=0, flow=p, w=p, dy=p, B=1, C=4, Hs=8, Ws=8, G=8, Dd=4, K=9, ddw=nul, scratch=nul, nscr=0,
             ws=p, nws=1 << 40, lib=L):
        return lib.gfn_refiner_input_bwd_det(grad_d, d_bs, f1, dtype, flow, w, nul, p, dy, p, ddw, nul, B, C, Hs, Ws, G, Dd, K, 1.25,
                                             scratch, nscr, ws, nws, nul)

    assert call(dtype=2) == _lib.ERR_INVALID_ARG and b"dtype" in L.gfn_last_error()
    for kw in (dict(grad_d=nul), dict(f1=nul), dict(flow=nul), dict(w=nul)):
        assert call(**kw) == _lib.ERR_INVALID_ARG and b"null pointer" in L.gfn_last_error(), kw
    for kw in (dict(B=-1), dict(C=0), dict(Hs=0), dict(Ws=0), dict(G=0), dict(Dd=-1), dict(K=-1), dict(d_bs=(2 * 4 + 4 + 9) * 64 - 1),
               dict(Hs=1 << 16, Ws=1 << 15, C=1)):
        assert call(**kw) == _lib.ERR_INVALID_ARG and b"bad size" in L.gfn_last_error(), kw
    assert call(B=65536) == _lib.ERR_INVALID_ARG
    assert call(ddw=p) == _lib.ERR_SCRATCH  # the partial sums' scratch, as on the plain entry point
    need = int(L.gfn_refiner_input_bwd_det_ws_bytes(1, 4, 8, 8))
    for kw in (dict(ws=nul), dict(ws=odd), dict(nws=need - 1), dict(nws=0)):
        assert call(**kw) == _lib.ERR_SCRATCH and b"refiner_input_bwd_det: ws" in L.gfn_last_error(), kw
    assert call(B=0, ws=nul, nws=0) == 0  # an empty batch is nothing to do
    with pytest.raises(_lib.GfnError, match=r"gfn_refiner_input_bwd_det failed \(-3\).*ws must be 8-byte aligned"):
        call(ws=odd, lib=_lib.checked())
    with pytest.raises(_lib.GfnError, match=r"gfn_refiner_input_bwd_det failed \(-3\)"):
        call(nws=need - 8, lib=_lib.checked())
    assert "gfn_refiner_input_bwd_det" in _lib.STATUS_FUNCS and "gfn_interp_bilinear_bwd" in _lib.STATUS_FUNCS
    assert "gfn_refiner_input_bwd_det_ws_bytes" not in _lib.STATUS_FUNCS
    assert L.gfn_refiner_input_bwd_det_ws_bytes.restype is ctypes.c_int64


def test_interp_bilinear_bwd_refuses_on_the_host():
    from gfnet_amd import _lib

    L = _lib.lib()
    p, nul = ctypes.c_void_p(64), ctypes.c_void_p(0)

    def call(g=p, out=p, BC=2, H=4, W=4, Ho=7, Wo=7, lib=L):
        return lib.gfn_interp_bilinear_bwd(g, out, BC, H, W, Ho, Wo, nul)

    for kw in (dict(g=nul), dict(out=nul), dict(BC=-1), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=-3)):
        assert call(**kw) == _lib.ERR_INVALID_ARG and b"interp_bilinear_bwd" in L.gfn_last_error(), kw
    for kw in (dict(H=1 << 16, W=1 << 15), dict(Ho=1 << 15, Wo=1 << 16)):
        assert call(**kw) == _lib.ERR_INVALID_ARG and b"plane too large" in L.gfn_last_error(), kw
    assert call(BC=0) == 0
    with pytest.raises(_lib.GfnError, match=r"gfn_interp_bilinear_bwd failed \(-1\)"):
        call(g=nul, lib=_lib.checked())


@pytest.mark.parametrize("flag", [False, True])
def test_deterministic_keyword_resolves_against_the_torch_flag(flag, restore_flag):
    from gfnet_amd import ops

    torch.use_deterministic_algorithms(flag)
    assert ops.resolve_deterministic(None) is flag
    assert ops.resolve_deterministic(True) is True and ops.resolve_deterministic(False) is False


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("keyword", [None, True, False])
def test_refiner_input_hands_the_resolved_value_to_its_autograd_function(monkeypatch, flag, keyword, restore_flag):
    """the value is resolved when the forward runs and travels as the function's last argument; ConvRefiner.assemble passes nothing,
    so the torch flag reaches it through the default"""
    from gfnet_amd import ops

    seen = []
    monkeypatch.setattr(ops._RefinerInputFn, "apply", staticmethod(lambda *a: seen.append(a) or "d"))
    t = dict(x=torch.randn(2, 4, 8, 8), y=torch.randn(2, 4, 8, 8), flow=torch.zeros(2, 2, 6, 6, requires_grad=True),
             w=torch.randn(3, 2, 1, 1), b=torch.randn(3))
    torch.use_deterministic_algorithms(flag)
    kw = {} if keyword is None else {"deterministic": keyword}
    assert ops.refiner_input(6, t["x"], t["y"], t["flow"], t["w"], t["b"], 1, **kw) == "d"
    torch.use_deterministic_algorithms(not flag)  # a later change of the flag does not reach a forward that has run
    assert len(seen) == 1 and len(seen[0]) == 10 and seen[0][-1] is (flag if keyword is None else keyword)


def test_backward_functions_take_the_keyword_and_have_no_cpu_path():
    from gfnet_amd import _lib, ops

    g = torch.zeros(2, 2 * 4 + 3 + 9, 6, 6)
    for det in (False, True):
        with pytest.raises(_lib.GfnError, match="no CPU path"):
            ops.refiner_input_bwd(g, torch.randn(2, 4, 8, 8), torch.zeros(2, 2, 6, 6), torch.randn(3, 2), 1, deterministic=det)


@pytest.mark.parametrize("grad", [False, True])
def test_resize_bilinear_refuses_cpu_tensors(grad):
    from gfnet_amd import _lib, ops

    x = torch.randn(1, 2, 4, 4, requires_grad=grad)
    with pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.resize_bilinear(x, (7, 7))
    with torch.no_grad(), pytest.raises(_lib.GfnError, match="no CPU path"):
        ops.resize_bilinear(x, 7)


class _Map:
    """what ReferenceBackbone's resize asks of the ViT map, so that the GPU branch can be reached without one"""

    def __init__(self, is_cuda, requires_grad):
        self.is_cuda, self.requires_grad = is_cuda, requires_grad


@pytest.mark.parametrize("is_cuda", [False, True])
@pytest.mark.parametrize("requires_grad", [False, True])
@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("grad_mode", [False, True])
def test_backbone_takes_the_gather_only_for_a_gpu_map_that_needs_a_gradient_under_the_flag(monkeypatch, is_cuda, requires_grad, flag,
                                                                                           grad_mode, restore_flag):
    from gfnet_amd import ops, reference_backbone

    calls = []
    monkeypatch.setattr(reference_backbone.F, "interpolate", lambda t, **kw: calls.append(("F.interpolate", kw)))
    monkeypatch.setattr(ops, "resize_bilinear", lambda t, size: calls.append(("ops.resize_bilinear", size)))
    torch.use_deterministic_algorithms(flag)
    with torch.set_grad_enabled(grad_mode):
        reference_backbone._resize_side(_Map(is_cuda, requires_grad), (14, 14))
    if is_cuda and requires_grad and flag and grad_mode:
        assert calls == [("ops.resize_bilinear", (14, 14))]
    else:
        assert calls == [("F.interpolate", dict(size=(14, 14), mode="bilinear", align_corners=False))]
