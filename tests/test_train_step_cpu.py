"""The fused training step (gfnet_amd.trainer, csrc/train_step.hip) without a GPU: the chunk-table builder, the CPU restatement
`reference_step` against torch's own GradScaler rule / clip_grad_norm_ / AdamW chained by hand in float64, the host checks of the
library entry, and the register budget of the kernels.  tests/test_train_step_gpu.py takes its shared cases from here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

CHUNK = 4096
HYPER = {"max_norm": 0.5, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "min_scale": 1.0}


def fresh_state(n, scale=65536.0):
    return {"exp_avg": [None] * n, "exp_avg_sq": [None] * n, "step": 0, "scale": scale, "tracker": 0}


def two_groups(n, split):
    """parameters 0 .. split-1 and split .. n-1 with different lr / weight_decay / betas / eps"""
    return [{"params": list(range(split)), "lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01},
            {"params": list(range(split, n)), "lr": 3e-3, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.1}]


# ---- the chunk table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1024, CHUNK])
def test_build_tables_covers_every_element_once(chunk):
    from gfnet_amd.trainer import build_tables

    sizes = [0, 1, 3, chunk - 1, chunk, chunk + 1, 0, 3 * chunk + 5, 2]
    aligned = [True, False, True, True, False, True, True, False, True]
    spans, chunks = build_tables(sizes, aligned, chunk)
    assert spans.shape == (len(sizes), 3) and chunks.shape[1] == 3
    assert chunks.shape[0] == sum((s + chunk - 1) // chunk for s in sizes)
    assert (chunks[:, 2] >= 1).all() and (chunks[:, 2] <= chunk).all()
    assert (chunks[:, 1] % chunk == 0).all()                        # a chunk starts on a chunk boundary: alignment carries over
    assert (np.diff(chunks[:, 0]) >= 0).all()                       # tensors in table order
    for t, (size, al) in enumerate(zip(sizes, aligned)):
        first_chunk, n_chunks, flag = (int(v) for v in spans[t])
        assert flag == int(al)
        mine = np.nonzero(chunks[:, 0] == t)[0]
        assert n_chunks == len(mine) == (size + chunk - 1) // chunk
        if size == 0:
            continue                                                # a zero-size tensor yields no chunk
        assert list(mine) == list(range(first_chunk, first_chunk + n_chunks))   # consecutive
        seen = np.zeros(size, dtype=np.int64)
        prev_end = 0
        for _, first, count in chunks[mine]:
            assert first == prev_end                                # ascending, no gap, no overlap
            assert first + count <= size                            # no chunk spans into the next tensor
            seen[first:first + count] += 1
            prev_end = first + count
        assert (seen == 1).all()
    with pytest.raises(ValueError):
        build_tables([5], [True], 1000)
    with pytest.raises(ValueError):
        build_tables([5, 6], [True], chunk)
    s0, c0 = build_tables([], [], chunk)
    assert s0.shape == (0, 3) and c0.shape == (0, 3)


def test_library_chunk_size_is_the_python_default():
    from gfnet_amd import _lib

    assert _lib.TS_CHUNK == CHUNK  # (_lib takes it from include/gfnet_hip.h, as csrc/train_step.hip does)


# ---- reference_step against torch itself ---------------------------------------------------------------------------------------------
def hand_chained(params, grads, groups, scale, max_norm, steps_before, moments):
    """grads / scale -> clip_grad_norm_ -> torch.optim.AdamW(foreach=False).step(), float64, one step; mutates params / moments"""
    leaves = [torch.nn.Parameter(p) for p in params]
    for leaf, g in zip(leaves, grads):
        leaf.grad = None if g is None else g / scale
    torch.nn.utils.clip_grad_norm_([lf for lf in leaves if lf.grad is not None], max_norm, foreach=False)
    opt = torch.optim.AdamW([{**{k: v for k, v in g.items() if k != "params"}, "params": [leaves[i] for i in g["params"] if grads[i] is not None]}
                             for g in groups], foreach=False)
    for i, leaf in enumerate(leaves):
        if grads[i] is not None:
            opt.state[leaf] = {"step": torch.tensor(float(steps_before)), "exp_avg": moments[0][i], "exp_avg_sq": moments[1][i]}
    opt.step()


def test_reference_step_equals_torch_chained_by_hand():
    from gfnet_amd.trainer import reference_step

    gen = torch.Generator().manual_seed(0)
    shapes = [(7,), (3, 5), (129,), (2, 2, 3), (11,)]
    n, scale = len(shapes), 1024.0
    params = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    groups = two_groups(n, 3)
    hyper = {**HYPER, "groups": groups}
    state = fresh_state(n, scale)
    want_p = [p.clone() for p in params]
    want_m = [[torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]]
    clipped = []
    for step in range(3):
        # gradient 4 is None throughout; the size of the gradients makes step 0 clip and step 2 not
        mag = (10.0, 0.3, 1e-3)[step]
        grads = [mag * scale * torch.randn(s, generator=gen, dtype=torch.float64) if i != 4 else None for i, s in enumerate(shapes)]
        params, state, stats = reference_step(params, grads, state, hyper)
        pnorm = float(torch.sqrt(sum((p ** 2).sum() for p in want_p[:4])))      # of the parameters BEFORE the update, gradient-less left out
        hand_chained(want_p, grads, groups, scale, HYPER["max_norm"], step, want_m)
        total = torch.sqrt(sum(((g / scale) ** 2).sum() for g in grads if g is not None))
        clipped.append(bool(total > HYPER["max_norm"]))
        assert abs(float(stats["grad_norm"]) - float(total)) <= 1e-12 * float(total)
        assert abs(float(stats["param_norm"]) - pnorm) <= 1e-12 * pnorm
        assert stats["found_inf"] is False and stats["nonfinite"] == [] and stats["grad_scale"] == scale
        assert state["step"] == step + 1 and state["scale"] == scale and state["tracker"] == step + 1
        for i in range(n):
            torch.testing.assert_close(params[i], want_p[i], rtol=1e-12, atol=1e-12)
            if i != 4:
                torch.testing.assert_close(state["exp_avg"][i], want_m[0][i], rtol=1e-12, atol=1e-12)
                torch.testing.assert_close(state["exp_avg_sq"][i], want_m[1][i], rtol=1e-12, atol=1e-12)
        assert state["exp_avg"][4] is None and torch.equal(params[4], want_p[4])
    assert clipped == [True, True, False]


def test_reference_step_param_norm_is_taken_before_the_update():
    from gfnet_amd.trainer import reference_step

    p = [torch.full((4,), 2.0, dtype=torch.float64)]
    g = [torch.ones(4, dtype=torch.float64)]
    _, _, stats = reference_step(p, g, fresh_state(1, 1.0), {**HYPER, "groups": [{"params": [0], "lr": 0.1, "betas": (0.9, 0.999), "eps": 1e-8,
                                                                                  "weight_decay": 0.0}]})
    assert float(stats["param_norm"]) == 4.0 and float(stats["grad_norm"]) == 2.0 and torch.equal(p[0], torch.full((4,), 2.0, dtype=torch.float64))


def test_reference_step_skips_on_a_nan_and_backs_the_scale_off():
    from gfnet_amd.trainer import reference_step

    gen = torch.Generator().manual_seed(1)
    params = [torch.randn(9, generator=gen, dtype=torch.float64) for _ in range(3)]
    hyper = {**HYPER, "groups": two_groups(3, 1)}
    state = fresh_state(3, 256.0)
    grads = [torch.randn(9, generator=gen, dtype=torch.float64) for _ in range(3)]
    params, state, _ = reference_step(params, grads, state, hyper)           # one clean step, so that there are moments to keep
    bad = [g.clone() for g in grads]
    bad[1][4] = float("nan")
    p2, s2, stats = reference_step(params, bad, state, hyper)
    assert stats["found_inf"] is True and stats["nonfinite"] == [1]
    assert s2["step"] == state["step"] == 1 and s2["scale"] == 128.0 and s2["tracker"] == 0
    for i in range(3):
        assert torch.equal(p2[i], params[i]) and torch.equal(s2["exp_avg"][i], state["exp_avg"][i])
        assert torch.equal(s2["exp_avg_sq"][i], state["exp_avg_sq"][i])


def test_reference_step_scale_rule():
    from gfnet_amd.trainer import reference_step

    p = [torch.zeros(3, dtype=torch.float64)]
    g = [torch.ones(3, dtype=torch.float64)]
    group = [{"params": [0], "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0}]
    hyper = {**HYPER, "groups": group, "growth_interval": 3}
    state = fresh_state(1, 8.0)
    seen = []
    for _ in range(7):
        p, state, _ = reference_step(p, g, state, hyper)
        seen.append((state["scale"], state["tracker"]))
    assert seen == [(8.0, 1), (8.0, 2), (16.0, 0), (16.0, 1), (16.0, 2), (32.0, 0), (32.0, 1)]    # grows exactly on the 3rd clean step
    inf = [torch.tensor([1.0, float("inf"), 1.0], dtype=torch.float64)]
    state = fresh_state(1, 1.5)
    for _ in range(3):                                                  # 1.5 -> 0.75 is floored at min_scale = 1, and stays there
        p, state, stats = reference_step(p, inf, state, hyper)
        assert stats["found_inf"] and state["scale"] == 1.0 and state["tracker"] == 0
    state = fresh_state(1, 8.0)
    _, state, _ = reference_step(p, inf, state, {**hyper, "min_scale": 6.0})
    assert state["scale"] == 6.0
    # no gradient anywhere: only the scale rule runs, with found_inf = 0
    _, state, stats = reference_step(p, [None], {**fresh_state(1, 8.0), "tracker": 2}, hyper)
    assert state["scale"] == 16.0 and state["step"] == 0 and not stats["found_inf"]


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_train_step():
    from gfnet_amd import _lib

    L = _lib.lib()
    assert hasattr(L, "gfn_train_step") and hasattr(L, "gfn_train_step_ws_bytes")
    assert {"gfn_train_step", "gfn_train_step_ws_bytes"} <= set(_lib.exported_symbols())
    # a 64-byte control block, 32 bytes of coefficients per tensor, three doubles per chunk; rounded up to 16
    assert L.gfn_train_step_ws_bytes(0, 0) == 64
    assert L.gfn_train_step_ws_bytes(3, 5) == (64 + 3 * 32 + 5 * 24 + 15) // 16 * 16
    assert L.gfn_train_step_ws_bytes(-1, 0) == 0


def test_train_step_entry_refuses_bad_arguments_without_a_gpu():
    """Every call has exactly one bad argument and is refused by the host checks before any launch (every pointer is a host buffer
    that no kernel may ever see)."""
    from gfnet_amd import _lib

    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    BIG = 1 << 40

    def call(tt=p, nt=2, ct=p, nc=3, state=p, max_norm=0.01, growth=2.0, backoff=0.5, interval=2000, zero=1, stats=p, ws=p, nws=BIG):
        return L.gfn_train_step(tt, nt, ct, nc, state, max_norm, growth, backoff, interval, zero, stats, ws, nws, None)

    bad = {"null tensor table": dict(tt=None), "null chunk table": dict(ct=None), "null state": dict(state=None), "null stats": dict(stats=None),
           "null workspace": dict(ws=None), "misaligned workspace": dict(ws=ctypes.c_void_p(p.value + 4)),
           "workspace one byte short": dict(nws=L.gfn_train_step_ws_bytes(2, 3) - 1), "n_tensors < 0": dict(nt=-1), "n_chunks < 0": dict(nc=-1),
           "more tensors than one finish workgroup takes": dict(nt=(1 << 20) + 1), "more chunks than the grid": dict(nc=(1 << 23) + 1),
           "chunks of no tensor": dict(nt=0), "max_norm < 0": dict(max_norm=-1.0), "max_norm nan": dict(max_norm=float("nan")),
           "growth < 1": dict(growth=0.5), "backoff = 0": dict(backoff=0.0), "backoff > 1": dict(backoff=2.0), "growth_interval = 0": dict(interval=0)}
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert L.gfn_last_error(), what
    assert b"workspace" in (call(nws=16), L.gfn_last_error())[1]
    assert b"2^20" in (call(nt=(1 << 20) + 1), L.gfn_last_error())[1]
    assert b"grid" in (call(nc=(1 << 23) + 1), L.gfn_last_error())[1]


def test_train_step_kernels_have_no_spills_and_no_scratch():
    obj = os.path.join(ROOT, "gfnet_amd", "csrc", "train_step.o")
    if not os.path.exists(obj):
        from gfnet_amd import build

        build.build()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), obj], capture_output=True, text=True, check=True).stdout
    rows = [ln for ln in out.splitlines() if "ts_" in ln]
    assert len(rows) == 3, out
    for ln in rows:
        f = ln.split()
        vals = {f[k]: f[k + 1] for k in range(len(f) - 1) if f[k] in ("spill", "sspill", "scratch")}
        assert vals == {"spill": "0", "sspill": "0", "scratch": "0"}, ln
        assert int(f[f.index("vgpr") + 1]) <= 128, ln   # at least four waves per SIMD


# ---- the public interface -----------------------------------------------------------------------------------------------------------
def test_stepper_refuses_cpu_and_half_parameters_without_a_gpu():
    from gfnet_amd._lib import GfnError
    from gfnet_amd.trainer import FusedAdamWStep

    with pytest.raises(GfnError, match="no CPU path"):
        FusedAdamWStep([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    with pytest.raises(ValueError):
        FusedAdamWStep([torch.nn.Parameter(torch.zeros(4))], lr=-1.0)
    with pytest.raises(ValueError):
        FusedAdamWStep([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, backoff_factor=0.0)
    with pytest.raises(ValueError, match="min_scale >= 1"):               # a scale below 1 could overflow finite gradients unseen
        FusedAdamWStep([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, min_scale=0.5)


def test_trainer_surface():
    import inspect

    from gfnet_amd import trainer

    sig = inspect.signature(trainer.FusedAdamWStep.__init__)
    got = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params_or_groups", "lr")}
    assert got == dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=0.01, init_scale=65536., growth_factor=2., backoff_factor=0.5,
                       growth_interval=2000, min_scale=1., zero_grads=True)
    assert list(inspect.signature(trainer.train_step).parameters)[:4] == ["train_batch", "model", "objective", "stepper"]
    assert list(inspect.signature(trainer.train_k_steps_cosine).parameters)[:7] == ["n_0", "k", "dataloader", "model", "objective", "stepper",
                                                                                     "lr_scheduler"]
    batch = {"a": 3, "b": "x"}
    assert trainer.to_cuda(batch) is batch and batch == {"a": 3, "b": "x"}      # nothing but tensors is touched
