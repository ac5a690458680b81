"""GPU: the fused training step (gfnet_amd.trainer.FusedAdamWStep on csrc/train_step.hip) against `reference_step`, the CPU restatement
built from torch's own clip_grad_norm_ / AdamW / scale rule that tests/test_train_step_cpu.py pins to torch in float64.

One list of parameter sizes throughout: below, at and above a float4, a 1024-element round of the workgroup and a chunk, plus a
three-chunk tensor with a tail.  The gradients are views into one flat buffer at element offsets that are 0, 1, 2, 3, 5, ... modulo
8, so that some tensors take the 16-byte path (with and without a tail shorter than a vector), the others the scalar path with
aligned parameters and moments against a misaligned gradient, single- and multi-chunk in both.

Tolerance of the parity tests (not fixed in advance): reference_step also runs in float32 on the CPU from the same inputs; per
tensor kind (p, exp_avg, exp_avg_sq) and step the bound is 4 x the largest deviation of that float32 run from the float64 run, and
not below 2^-22 * max(|ref|, lr) per element.  The factor 4 covers a different summation order of the norm and the roundings of
another operation order where ATen's CPU and device kernels differ.  No element is left out."""
import copy

import pytest
import torch
import torch.nn as nn

from conftest import load_golden
from test_train_step_cpu import CHUNK, fresh_state, two_groups

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
RESIDUES = [0, 1, 2, 3, 5, 0, 7, 4, 0, 6, 0]      # gradient start, in elements modulo 8: 0 and 4 are 16-byte aligned
VECTOR = [r % 4 == 0 for r in RESIDUES]
NO_GRAD = len(SIZES)                               # one more parameter, of 17 elements, never gets a gradient
SPLIT = 6
SCALER = {"max_norm": 50.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "min_scale": 1.0}
KINDS = ("p", "exp_avg", "exp_avg_sq")


def dev_state(stepper):
    """(scale, tracker, step) as the device holds them"""
    s = stepper.state_dict()["scaler"]["device_state"].cpu()
    return float(s[0:1].view(torch.float32)[0]), int(s[1]), int(s[2:4].view(torch.int64)[0])


class Rig:
    """the parameters, their gradient views, a FusedAdamWStep over them and the CPU inputs of reference_step"""

    def __init__(self, seed=0, init_scale=65536.0, zero_grads=True, init=None, **scaler):
        from gfnet_amd.trainer import FusedAdamWStep

        gen = torch.Generator().manual_seed(seed)
        self.sizes = SIZES + [17]
        self.n = len(self.sizes)
        self.init = [torch.randn(s, generator=gen) for s in self.sizes] if init is None else [t.detach().cpu().clone() for t in init]
        self.params = [nn.Parameter(t.clone().cuda()) for t in self.init]
        self.offsets, cur = [], 0
        for s, r in zip(SIZES, RESIDUES):
            pos = cur + (r - cur) % 8
            self.offsets.append(pos)
            cur = pos + s
        self.flat = torch.zeros(cur + 8, device="cuda")
        assert self.flat.data_ptr() % 16 == 0
        for p, o, s in zip(self.params, self.offsets, SIZES):
            p.grad = self.flat[o:o + s]
            assert (p.grad.data_ptr() % 16 == 0) == (o % 4 == 0) and p.data_ptr() % 16 == 0
        self.groups = two_groups(self.n, SPLIT)
        self.hyper = {**SCALER, **scaler, "groups": self.groups}
        named = [{**{k: v for k, v in g.items() if k != "params"}, "params": [(f"w{i}", self.params[i]) for i in g["params"]]} for g in self.groups]
        kw = {k: self.hyper[k] for k in ("max_norm", "growth_factor", "backoff_factor", "growth_interval", "min_scale")}
        self.stepper = FusedAdamWStep(named, lr=1.0, init_scale=init_scale, zero_grads=zero_grads, **kw)
        self.lr = [next(g["lr"] for g in self.groups if i in g["params"]) for i in range(self.n)]
        self.ref = {dt: {"params": [t.to(dt) for t in self.init], "state": fresh_state(self.n, max(init_scale, self.hyper["min_scale"]))}
                    for dt in (torch.float64, torch.float32)}

    def make_grads(self, k, mag):
        """fresh random SCALED gradients of step k as CPU fp32 tensors (None for the parameter that has none)"""
        gen = torch.Generator().manual_seed(1000 + k)
        scale = self.ref[torch.float64]["state"]["scale"]
        return [None if self.params[i].grad is None else (mag * scale) * torch.randn(self.sizes[i], generator=gen) for i in range(self.n)]

    def load_grads(self, grads):
        for p, g in zip(self.params, grads):
            if g is not None:
                p.grad.copy_(g.cuda())

    def step(self, grads):
        """one GPU step and one reference step per dtype on the same gradients; returns the float64 stats"""
        from gfnet_amd.trainer import reference_step

        self.load_grads(grads)
        self.stepper.step()
        for dt, r in self.ref.items():
            r["params"], r["state"], stats = reference_step(r["params"], [None if g is None else g.to(dt) for g in grads], r["state"], self.hyper)
            r["stats"] = stats
        return self.ref[torch.float64]["stats"]

    def got(self, kind, i):
        if kind == "p":
            return self.params[i].detach().cpu()
        st = self.stepper.state.get(self.params[i], {})
        return st[kind].detach().cpu() if kind in st else None

    def want(self, kind, i, dt=torch.float64):
        r = self.ref[dt]
        return r["params"][i] if kind == "p" else r["state"][kind][i]

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: [None if self.got(k, i) is None else self.got(k, i).clone() for i in range(self.n)] for k in KINDS}

    def worst_ratio(self):
        """largest |got - ref64| / bound over every element of every tensor, per kind, with the calibrated bound of the module docstring"""
        worst = {}
        for kind in KINDS:
            idx = [i for i in range(self.n) if self.want(kind, i) is not None]
            dev = max(float((self.want(kind, i, torch.float32).double() - self.want(kind, i)).abs().max()) for i in idx)
            w = 0.0
            for i in range(self.n):
                ref, got = self.want(kind, i), self.got(kind, i)
                assert (ref is None) == (got is None), f"{kind}[{i}]: state present on one side only"
                if ref is None:
                    continue
                assert torch.isfinite(got).all(), f"{kind}[{i}]: non-finite"
                bound = torch.clamp(2.0 ** -22 * torch.clamp(ref.abs(), min=self.lr[i]), min=4.0 * dev)
                w = max(w, float(((got.double() - ref).abs() / bound).max()))
            worst[kind] = w
        return worst


@pytest.fixture(scope="module")
def parity_run():
    """4 steps with fresh gradients; gradient norms 155, 15.5, 310, 31 against max_norm = 50: clipped, not, clipped, not"""
    rig = Rig()
    records = []
    for k, mag in enumerate((1.0, 0.1, 2.0, 0.2)):
        stats = rig.step(rig.make_grads(k, mag))
        torch.cuda.synchronize()
        records.append({"ratios": rig.worst_ratio(), "ref": stats, "got": {k2: v.clone().cpu() for k2, v in rig.stepper.last_stats.items()},
                        "dev_state": dev_state(rig.stepper), "ref_state": {k2: rig.ref[torch.float64]["state"][k2] for k2 in ("scale", "tracker", "step")},
                        "grads_after": float(rig.flat.abs().max())})
    return rig, records


def test_parity_with_the_float64_reference(parity_run):
    rig, records = parity_run
    for k, rec in enumerate(records):
        print(f"train step {k}: worst err / bound {rec['ratios']}, clip_coef {rec['ref']['clip_coef']:.4f}")
    assert [rec["ref"]["clip_coef"] < 1.0 for rec in records] == [True, False, True, False]
    for k, rec in enumerate(records):
        for kind, r in rec["ratios"].items():
            assert r <= 1.0, f"step {k}, {kind}: {r:.2f} x the bound"
        assert rec["grads_after"] == 0.0                             # zero_grads: the next step's zero_grad
    # the parameter without a gradient: untouched, no moments
    assert torch.equal(rig.got("p", NO_GRAD), rig.init[NO_GRAD]) and rig.got("exp_avg", NO_GRAD) is None
    # the paths the sizes were chosen for
    t = rig.stepper._tensors
    assert [bool(v) for v in t["vec16"]] == VECTOR and len(t) == len(SIZES)
    assert list(t["n_chunks"]) == [1] * 8 + [1, 2, 3]


def test_logged_scalars(parity_run):
    _, records = parity_run
    for k, rec in enumerate(records):
        ref, got = rec["ref"], rec["got"]
        for name in ("grad_norm", "param_norm"):
            assert got[name].dim() == 0
            assert abs(float(got[name]) - float(ref[name])) <= 1e-6 * float(ref[name]), (k, name, float(got[name]), float(ref[name]))
        assert float(got["grad_scale"]) == ref["grad_scale"] == 65536.0 and float(got["found_inf"]) == 0.0
        assert got["nonfinite"].shape == (len(SIZES),) and not got["nonfinite"].any()
        assert rec["dev_state"] == (rec["ref_state"]["scale"], rec["ref_state"]["tracker"], rec["ref_state"]["step"]) == (65536.0, k + 1, k + 1)
        assert abs(float(got["clip_coef"]) - ref["clip_coef"]) <= 1e-6 * ref["clip_coef"]


@pytest.mark.parametrize("zero_grads", [True, False])
def test_overflow_step_changes_nothing_but_the_scale(zero_grads):
    rig = Rig(seed=1, zero_grads=zero_grads)

    def overflow(k):
        grads = rig.make_grads(k, 0.5)
        grads[4][500] = float("inf")                    # a mid-sized tensor on the scalar path
        grads[10][-1] = float("nan")                    # the last element of the three-chunk tensor: the tail of its last chunk
        before, state_before = rig.snapshot(), dev_state(rig.stepper)
        stats = rig.step(grads)
        after = rig.snapshot()
        assert stats["found_inf"] and float(rig.stepper.last_stats["found_inf"]) == 1.0
        assert rig.stepper.nonfinite_names() == ["w4", "w10"]
        scale, tracker, step = dev_state(rig.stepper)
        assert (scale, tracker, step) == (state_before[0] * 0.5, 0, state_before[2])
        assert float(rig.stepper.last_stats["grad_scale"]) == state_before[0]
        for kind in KINDS:
            for i in range(rig.n):
                a, b = before[kind][i], after[kind][i]
                if b is None:
                    continue
                if a is None:                                       # moments allocated by this very step: still zero
                    assert not b.any(), (kind, i)
                else:
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, i)
        for i, g in enumerate(grads[:-1]):
            left = rig.params[i].grad.cpu()
            if zero_grads:
                assert not left.view(torch.int32).any(), i
            else:                                                  # exactly as they came in, still scaled, the inf and the nan included
                assert torch.equal(left.view(torch.int32), g.view(torch.int32)), i
        return step

    def clean(k):
        rig.step(rig.make_grads(k, 0.5))
        torch.cuda.synchronize()
        for kind, r in rig.worst_ratio().items():
            assert r <= 1.0, f"clean step {k}, {kind}: {r:.2f} x the bound"
        assert rig.stepper.nonfinite_names() == []
        return dev_state(rig.stepper)[2]

    assert overflow(0) == 0
    assert clean(1) == 1 == rig.ref[torch.float64]["state"]["step"]      # the next clean step uses step count 1, not 2
    assert overflow(2) == 1                                               # now with moments to keep
    assert clean(3) == 2
    assert dev_state(rig.stepper)[0] == 65536.0 / 4


def test_large_finite_gradients_are_not_an_overflow():
    """g = +-1e30 under scale 1: the squares overflow fp32 (a float32 norm is inf, clip_grad_norm_ then zeroes the step), the double
    accumulation does not.  The float32 CPU run cannot calibrate this case, so the bounds are worked out, in units of u = 2^-24 (one
    fp32 rounding, relative).  gu = g * clip_coef: 2u (clip_coef rounded to fp32, one product).  exp_avg = (1 - beta1) * gu: 4u (the
    weight as fp32, one product).  exp_avg_sq = (1 - beta2) * gu * gu: 2 * 2u + 3u = 7u.  Both <= 2^-21.  The first step is
    -(lr / bc1) * m / (sqrt(v) / bc2_sqrt + eps), about lr in size; the error of gu cancels between m and sqrt(v), what is left is 1u
    (step size as fp32) + 2u (m) + 1u (product) + 2.5u (sqrt(v)) + 2u (bc2_sqrt as fp32, division) + 0.5u (+ eps) + 1u (division) =
    10u, so |p - ref| <= 1u |p| (decay) + 10u lr + 1u |p| (the last add) <= 12u max(|p|, lr) <= 2^-20 max(|ref|, lr)."""
    from gfnet_amd.trainer import reference_step

    rig = Rig(seed=2, init_scale=1.0)
    gen = torch.Generator().manual_seed(7)
    grads = [None if rig.params[i].grad is None else torch.where(torch.rand(s, generator=gen) < 0.5, -1e30, 1e30).float()
             for i, s in enumerate(rig.sizes)]
    rig.load_grads(grads)
    rig.stepper.step()
    torch.cuda.synchronize()
    r = rig.ref[torch.float64]
    params, state, stats = reference_step(r["params"], [None if g is None else g.double() for g in grads], r["state"], rig.hyper)
    got = rig.stepper.last_stats
    assert not stats["found_inf"] and float(got["found_inf"]) == 0.0 and not got["nonfinite"].any()
    total = float(stats["grad_norm"])
    assert 1e32 < total < 1e33 and abs(float(got["grad_norm"]) - total) <= 1e-6 * total
    assert dev_state(rig.stepper) == (1.0, 1, 1)
    worst = 0.0
    for i in range(len(SIZES)):
        p = rig.got("p", i)
        assert torch.isfinite(p).all() and not torch.equal(p, rig.init[i])                     # the step is taken
        bound = 2.0 ** -20 * torch.clamp(params[i].abs(), min=rig.lr[i])
        worst = max(worst, float(((p.double() - params[i]).abs() / bound).max()))
        for kind in ("exp_avg", "exp_avg_sq"):
            m, want = rig.got(kind, i).double(), state[kind][i]
            assert ((m - want).abs() <= 2.0 ** -21 * want.abs()).all(), (kind, i)
    print(f"1e30 gradients: worst err / bound {worst:.3f}")
    assert worst <= 1.0


def test_scaler_rule():
    rig = Rig(seed=3, growth_interval=3, init_scale=1024.0)
    used = []
    for k in range(4):
        rig.step(rig.make_grads(k, 0.1))
        used.append(float(rig.stepper.last_stats["grad_scale"]))
    assert used == [1024.0, 1024.0, 1024.0, 2048.0]                  # doubled exactly after the third clean step
    assert dev_state(rig.stepper) == (2048.0, 1, 4)
    assert rig.ref[torch.float64]["state"]["scale"] == 2048.0
    rig = Rig(seed=3, init_scale=1.5)
    grads = rig.make_grads(0, 0.1)
    grads[0][0] = float("inf")
    rig.step(grads)
    assert dev_state(rig.stepper) == (1.0, 0, 0)                     # min_scale, not 0.75
    x = torch.full((), 3.0, device="cuda")
    assert float(rig.stepper.scale_loss(x)) == 3.0


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        rig = Rig(seed=4)
        stats = []
        for k, mag in enumerate((1.0, 0.1)):
            rig.load_grads(rig.make_grads(k, mag))
            rig.stepper.step()
            stats.append(rig.stepper._stats.clone().cpu())
        runs.append((rig.snapshot(), stats))
    (a, sa), (b, sb) = runs
    for kind in KINDS:
        for x, y in zip(a[kind], b[kind]):
            assert (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)), kind
    for x, y in zip(sa, sb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_tables_are_rebuilt_when_gradients_move():
    rig = Rig(seed=5)
    rig.step(rig.make_grads(0, 1.0))
    key0 = rig.stepper._key
    rig.step(rig.make_grads(1, 0.1))
    assert rig.stepper._key is key0                                  # a steady run never rebuilds
    moments = {i: rig.stepper.state[rig.params[i]]["exp_avg"].data_ptr() for i in range(len(SIZES))}
    rig.params[3].grad = torch.zeros(SIZES[3], device="cuda")        # a new gradient tensor
    rig.params[6].grad = None                                        # set_to_none
    rig.step(rig.make_grads(2, 1.0))
    torch.cuda.synchronize()
    assert rig.stepper._key is not key0 and len(rig.stepper._tensors) == len(SIZES) - 1
    for kind, r in rig.worst_ratio().items():
        assert r <= 1.0, f"after the rebuild, {kind}: {r:.2f} x the bound"
    assert moments == {i: rig.stepper.state[rig.params[i]]["exp_avg"].data_ptr() for i in range(len(SIZES))}    # moments kept
    rig.params[6].grad = rig.flat[rig.offsets[6]:rig.offsets[6] + SIZES[6]]
    rig.step(rig.make_grads(3, 0.1))
    torch.cuda.synchronize()
    assert len(rig.stepper._tensors) == len(SIZES)
    for kind, r in rig.worst_ratio().items():
        assert r <= 1.0, f"with the gradient back, {kind}: {r:.2f} x the bound"


def test_state_dict_round_trip_resumes_bit_identically():
    whole, part = Rig(seed=6), Rig(seed=6)
    for k, mag in enumerate((1.0, 0.1, 2.0)):
        whole.load_grads(whole.make_grads(k, mag))
        whole.stepper.step()
    for k, mag in enumerate((1.0, 0.1)):
        part.load_grads(part.make_grads(k, mag))
        part.stepper.step()
    saved = copy.deepcopy(part.stepper.state_dict())
    # a fresh stepper over copies of the parameters, with the same gradient layout (the norm's summation order depends on it)
    rest = Rig(seed=6, init=part.params, init_scale=4.0)
    fresh, resumed = rest.params, rest.stepper
    assert dev_state(resumed) == (4.0, 0, 0)
    resumed.load_state_dict(saved)
    assert dev_state(resumed) == dev_state(part.stepper) == (65536.0, 2, 2)
    rest.load_grads(whole.make_grads(2, 2.0))
    resumed.step()
    torch.cuda.synchronize()
    for i in range(whole.n):
        assert torch.equal(fresh[i].detach().view(torch.int32), whole.params[i].detach().view(torch.int32)), i
        for kind in ("exp_avg", "exp_avg_sq"):
            a, b = resumed.state.get(fresh[i], {}).get(kind), whole.stepper.state.get(whole.params[i], {}).get(kind)
            assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32)), (kind, i)
    assert dev_state(resumed) == dev_state(whole.stepper)
    assert torch.equal(resumed._stats[:8].view(torch.int32), whole.stepper._stats[:8].view(torch.int32))


def test_a_cosine_scheduler_drives_the_learning_rate():
    rig = Rig(seed=8)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(rig.stepper, T_max=4)
    for k in range(2):
        rig.step(rig.make_grads(k, 0.1))
        sched.step()
        for g_ref, g in zip(rig.groups, rig.stepper.param_groups):
            g_ref["lr"] = g["lr"]                                      # the reference follows the schedule
        rig.lr = [next(g["lr"] for g in rig.groups if i in g["params"]) for i in range(rig.n)]
    assert rig.stepper.param_groups[0]["lr"] < 1e-2
    rig.step(rig.make_grads(2, 0.1))
    torch.cuda.synchronize()
    for kind, r in rig.worst_ratio().items():
        assert r <= 1.0, f"{kind}: {r:.2f} x the bound"


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_g12_model():
    from gfnet_amd.trainer import FusedAdamWStep, reference_step, train_step
    from test_train_cpu import SCALES, g12_pyramids, weighted_loss
    from test_train_gpu import g12_model

    g = load_golden("g12_train_grads")
    torch.manual_seed(0)
    model = g12_model(g)
    twin = copy.deepcopy(model)
    pyr0, pyr1 = g12_pyramids(g, "cuda")
    hw = tuple(int(v) for v in g["image_hw"])
    lr, wd, max_norm = 1e-3, 0.01, 0.01
    stepper = FusedAdamWStep(model.named_parameters(), lr=lr, weight_decay=wd, max_norm=max_norm)
    stepper.scale_loss(weighted_loss(g, model.forward_pyramids(pyr0, pyr1, hw))).backward()
    named = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    assert len(named) >= 50                                                 # five refiners, ten or more tensors each
    scale = 65536.0
    grads = {n: p.grad.detach().clone() for n, p in named}
    before = {n: p.detach().clone() for n, p in named}
    for n, p in twin.named_parameters():
        if n in grads:
            p.grad = grads[n] / scale
    stepper.step()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm, foreach=False)
    torch.optim.AdamW(twin.parameters(), lr=lr, weight_decay=wd, foreach=False).step()
    torch.cuda.synchronize()
    assert float(stepper.last_stats["found_inf"]) == 0.0 and stepper.nonfinite_names() == []
    # calibration: reference_step in float64 and in float32 on the CPU from the same parameters and gradients
    names = [n for n, _ in named]
    hyper = {"max_norm": max_norm, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "min_scale": 1.0,
             "groups": [{"params": list(range(len(names))), "lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": wd}]}
    ref, stats = {}, {}
    for dt in (torch.float64, torch.float32):
        ref[dt], _, stats[dt] = reference_step([before[n].cpu().to(dt) for n in names], [grads[n].cpu().to(dt) for n in names],
                                           fresh_state(len(names)), hyper)
    dev = max(float((a.double() - b).abs().max()) for a, b in zip(ref[torch.float32], ref[torch.float64]))
    twin_p = dict(twin.named_parameters())
    worst = {"vs float64": 0.0, "vs torch on the device": 0.0}
    for i, (n, p) in enumerate(named):
        r64 = ref[torch.float64][i]
        bound = torch.clamp(2.0 ** -22 * torch.clamp(r64.abs(), min=lr), min=4.0 * dev)
        got = p.detach().cpu().double()
        worst["vs float64"] = max(worst["vs float64"], float(((got - r64).abs() / bound).max()))
        worst["vs torch on the device"] = max(worst["vs torch on the device"],
                                              float(((got - twin_p[n].detach().cpu().double()).abs() / bound).max()))
        assert not p.grad.any()                                              # zeroed, still allocated
    print(f"G12 model, one step: worst err / bound {worst}")
    total = float(stats[torch.float64]["grad_norm"])
    assert abs(float(stepper.last_stats["grad_norm"]) - total) <= 1e-6 * total
    assert worst["vs float64"] <= 1.0 and worst["vs torch on the device"] <= 1.0

    # train_step: the loss comes back as a detached device scalar, and nothing in the call synchronises
    weights = {(s, itr, kind): torch.from_numpy(g[f"w{kind}.{s}.{itr}"]).cuda() for s in SCALES for itr in range(1, int(g["num_itr"][SCALES.index(s)]) + 1)
               for kind in ("flow", "cert")}

    class Wrapped(nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def forward(self, batch):
            return self.net.forward_pyramids(batch["pyr0"], batch["pyr1"], hw)

    def objective(out, batch):
        loss = torch.zeros((), device="cuda")
        for s in SCALES:
            for itr, d in out[s].items():
                loss = loss + (weights[(s, itr, "flow")] * d["flow"]).sum() + (weights[(s, itr, "cert")] * d["certainty"]).sum()
        return loss

    batch = {"pyr0": {s: t.detach() for s, t in pyr0.items()}, "pyr1": {s: t.detach() for s, t in pyr1.items()}}
    key = stepper._key
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = train_step(batch, Wrapped(model), objective, stepper)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    loss = res["train_loss"]
    assert loss.is_cuda and loss.dim() == 0 and loss.grad_fn is None and not loss.requires_grad
    assert set(res) == {"train_out", "train_loss"} and res["train_out"]["1"][1]["flow"].is_cuda
    assert stepper._key == key                                               # zero_grads kept the gradients: no rebuild
    assert torch.isfinite(loss).item() and dev_state(stepper)[2] == 2


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gfnet_amd._lib import GfnError
    from gfnet_amd.trainer import FusedAdamWStep

    with pytest.raises(GfnError, match="fp32"):
        FusedAdamWStep([nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float16))], lr=1e-3)
    with pytest.raises(GfnError, match="fp32"):
        FusedAdamWStep([nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.bfloat16))], lr=1e-3)
    with pytest.raises(GfnError, match="no CPU path"):
        FusedAdamWStep([nn.Parameter(torch.zeros(8, device="cuda")), nn.Parameter(torch.zeros(8))], lr=1e-3)
    p = nn.Parameter(torch.zeros(4, 6, device="cuda"))
    stepper = FusedAdamWStep([p], lr=1e-3)
    p.grad = torch.zeros(6, 4, device="cuda").t()
    with pytest.raises(GfnError, match="not contiguous"):
        stepper.step()
    q = nn.Parameter(torch.zeros(6, 4, device="cuda").t())
    with pytest.raises(GfnError, match="contiguous"):
        FusedAdamWStep([q], lr=1e-3)
    with pytest.raises(ValueError, match="closure"):
        stepper.step(lambda: None)
    p.grad = torch.zeros(4, 6, device="cuda").to_sparse()
    with pytest.raises(GfnError, match="dense gradients only"):
        stepper.step()
    # a gradient of another dtype in a block of the same address and size is seen, not handed to the kernel
    p.grad = None
    p.grad = torch.zeros(4, 6, device="cuda")
    stepper.step()
    key = stepper._key
    assert key[0][3] is torch.float32 and key[0][4] is True
    p.grad = None
    stepper.step()                                                       # no gradient anywhere: only the scale rule runs
    assert dev_state(stepper) == (65536.0, 2, 1)                         # after the one real step above: tracker + 1, step count kept


def test_train_k_steps_cosine_steps_the_scheduler_once():
    from gfnet_amd.trainer import FusedAdamWStep, train_k_steps_cosine

    torch.manual_seed(0)
    class OnBatch(nn.Linear):
        def forward(self, batch):
            return super().forward(batch["x"])

    model = OnBatch(5, 3).cuda().eval()
    stepper = FusedAdamWStep(model.named_parameters(), lr=1e-2, max_norm=1.0, init_scale=256.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(stepper, T_max=10)
    batches = iter([{"x": torch.randn(4, 5), "y": torch.randn(4, 3), "tag": "cpu batch"} for _ in range(3)])
    before = [p.detach().clone() for p in model.parameters()]
    res = train_k_steps_cosine(7, 3, batches, model, lambda out, b: ((out - b["y"]) ** 2).mean(), stepper, sched)
    assert model.training                                                # model.train(True) before every step
    assert res["train_out"].is_cuda and res["train_loss"].grad_fn is None
    assert dev_state(stepper) == (256.0, 3, 3)
    assert sched.last_epoch == 1 and stepper.param_groups[0]["lr"] < 1e-2    # one scheduler step after the k steps
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(not p.grad.any() for p in model.parameters())
