"""trainer/train.py of the reference: `to_cuda` (:7-11), `train_step` (:29-43), `train_k_steps_cosine` (:45-64), without wandb, tqdm
or gfnet_configs, and with everything the reference does between `backward()` and the next `zero_grad()` on csrc/train_step.hip.

`FusedAdamWStep` stands where the reference has a `torch.optim.AdamW` and a `torch.amp.GradScaler`: `step()` is the unscale, the
gradient and parameter norms of `log_param_statistics` (:13-27), `clip_grad_norm_`, the AdamW update, the scale update with the
floor of :40-41 and the next step's `zero_grad`, as three launches and no host synchronisation.  What the reference sends to wandb is
left in `FusedAdamWStep.last_stats` as device tensors.  `reference_step` restates the same step with torch's own optimizer on the CPU,
in any dtype: the oracle of the tests.  There is no CPU path for the step itself.

Deliberately different from the torch sequence:
  * after `step()` the gradients are zero (`zero_grads=True`, the default: this is the next step's `optimizer.zero_grad()`, and it keeps
    them allocated, so the device tables are built once), or, with `zero_grads=False`, exactly as `backward()` left them, still
    scaled -- torch leaves them unscaled and clipped;
  * AdamW's step count is one device scalar for all parameters (a skipped step must not advance it and the host does not look), where
    torch keeps one per parameter: a parameter whose first gradient comes late starts with the shared count, not with 1;
  * `train_step` returns the loss as a 0-dim device tensor, where the reference calls `.item()`.
"""
import numpy as np
import torch

from .. import _lib

_TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"), ("lr", "<f8"), ("wd", "<f8"),
                       ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("first_chunk", "<i4"), ("n_chunks", "<i4"), ("vec16", "<i4"),
                       ("reserved", "<i4")])                                      # gfn_ts_tensor
_CHUNK_DT = np.dtype([("tensor", "<i4"), ("count", "<i4"), ("first", "<i8")])     # gfn_ts_chunk
_STATE_DT = np.dtype([("scale", "<f4"), ("tracker", "<i4"), ("step", "<i8"), ("min_scale", "<f4"), ("reserved", "<i4", (3,))])
assert _TENSOR_DT.itemsize == 96 and _CHUNK_DT.itemsize == 16 and _STATE_DT.itemsize == _lib.TS_STATE_BYTES


def build_tables(numels, aligned, chunk=_lib.TS_CHUNK):
    """The chunk table of gfn_train_step for tensors of `numels` elements: every workgroup gets at most `chunk` elements of one tensor,
    a tensor's chunks are consecutive and ascending, a tensor of no elements gets none.  `aligned[i]` says whether all four pointers
    of tensor i are 16-byte aligned.  Returns (spans, chunks): spans (n, 3) int64 rows (first chunk, number of chunks, 16-byte path
    allowed) per tensor, chunks (m, 3) int64 rows (tensor index, first element, count) per workgroup."""
    if chunk <= 0 or chunk % 1024:
        raise ValueError(f"build_tables: chunk = {chunk} must be a positive multiple of 1024 elements (256 threads x float4)")
    numels = np.asarray(list(numels), dtype=np.int64).reshape(-1)
    flags = np.asarray([bool(a) for a in aligned], dtype=np.int64).reshape(-1)
    if numels.shape != flags.shape:
        raise ValueError(f"build_tables: {numels.size} sizes, {flags.size} alignment flags")
    if (numels < 0).any():
        raise ValueError("build_tables: negative size")
    per = (numels + chunk - 1) // chunk
    first_chunk = np.cumsum(per) - per
    tensor = np.repeat(np.arange(numels.size, dtype=np.int64), per)
    first = (np.arange(tensor.size, dtype=np.int64) - first_chunk[tensor]) * chunk
    count = np.minimum(chunk, numels[tensor] - first)
    return np.stack((first_chunk, per, flags), axis=1), np.stack((tensor, first, count), axis=1)


class FusedAdamWStep(torch.optim.Optimizer):
    """AdamW (amsgrad=False, maximize=False) + GradScaler + clip_grad_norm_ + the statistics of log_param_statistics in one fused step.

    `params_or_groups` is what a torch optimizer takes: parameters, `named_parameters()` or parameter groups; `param_groups` has the
    usual keys, so a torch lr scheduler drives it unchanged (`lr` is read from the groups at every step).  fp32 CUDA parameters with
    dense, contiguous fp32 gradients only."""

    def __init__(self, params_or_groups, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=0.01, init_scale=65536.,
                 growth_factor=2., backoff_factor=0.5, growth_interval=2000, min_scale=1., zero_grads=True):
        if not lr >= 0.0 or not eps >= 0.0 or not weight_decay >= 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdamWStep: bad hyperparameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        if not max_norm >= 0.0 or not growth_factor >= 1.0 or not 0.0 < backoff_factor <= 1.0 or int(growth_interval) < 1 \
                or not init_scale > 0.0 or not min_scale >= 1.0:
            # a scale below 1 makes 1 / scale exceed 1: a finite gradient could then overflow in g * (1 / scale) without being found
            raise ValueError("FusedAdamWStep: needs max_norm >= 0, growth_factor >= 1, 0 < backoff_factor <= 1, growth_interval >= 1, "
                             "init_scale > 0 and min_scale >= 1")
        super().__init__(params_or_groups, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.max_norm, self.growth_factor, self.backoff_factor = float(max_norm), float(growth_factor), float(backoff_factor)
        self.growth_interval, self.zero_grads = int(growth_interval), bool(zero_grads)
        self._device = None
        for group in self.param_groups:
            for p in group["params"]:
                self._check_param(p)
        if self._device is None:
            raise ValueError("FusedAdamWStep: no parameters")
        host = np.zeros(1, dtype=_STATE_DT)
        host["scale"], host["min_scale"] = max(init_scale, min_scale), min_scale
        self._dev_state = self._upload(host).view(torch.int32)       # scale, tracker, step (2 words), min_scale, 3 reserved
        self._scale = self._dev_state[0:1].view(torch.float32)[0]    # 0-dim views of the device state
        self._key = self._hyper = None
        self._tensors = self._tensor_table = self._chunk_table = self._ws = self._stats = None
        self._n_chunks, self._names = 0, []
        self.last_stats = {}

    # ---- what the caller sees ---------------------------------------------------------------------------------------------------
    def scale_loss(self, loss):
        """loss * scale (grad_scaler.scale(l), trainer/train.py:33): a device multiply, no synchronisation"""
        return loss * self._scale

    def nonfinite_names(self):
        """Names of the parameters whose gradient held an inf or nan in the last step (log_param_statistics' `nan_inf_names`).  This
        read of the flags is the caller's synchronisation."""
        if not self.last_stats:
            return []
        flags = self.last_stats["nonfinite"].cpu().tolist()
        return [name for name, f in zip(self._names, flags) if f]

    def state_dict(self):
        sd = super().state_dict()
        sd["scaler"] = {"device_state": self._dev_state.clone(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                        "growth_interval": self.growth_interval}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        sc = state_dict["scaler"]
        dev = sc["device_state"]
        if dev.dtype != torch.int32 or dev.numel() != self._dev_state.numel():
            raise ValueError("FusedAdamWStep.load_state_dict: 'device_state' is not this class's (scale, tracker, step, min_scale) block")
        self._dev_state.copy_(dev)
        self.growth_factor, self.backoff_factor = float(sc["growth_factor"]), float(sc["backoff_factor"])
        self.growth_interval = int(sc["growth_interval"])
        self._key = None                                         # the moments are new tensors: rebuild the tables

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdamWStep.step takes no closure: the loss has to be scaled with scale_loss() before backward()")
        entries = [(gi, i, p) for gi, group in enumerate(self.param_groups) for i, p in enumerate(group["params"]) if p.grad is not None]
        for _, _, p in entries:
            if p.grad.layout is not torch.strided:               # (a sparse gradient has no data_ptr to compare)
                raise _lib.GfnError(f"FusedAdamWStep: a parameter of shape {tuple(p.shape)} has a {p.grad.layout} gradient; dense gradients only")
        # what the tables were built from and checked for: a gradient of another dtype or layout in a recycled block must not pass unseen
        key = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel(), p.grad.dtype, p.grad.is_contiguous()) for _, _, p in entries)
        hyper = tuple((g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"]) for g in self.param_groups)
        if key != self._key:
            self._rebuild(entries, key)
            self._hyper = None
        if hyper != self._hyper:
            self._upload_hyper(entries, hyper)
        n = len(entries)
        if self._device.index is not None and self._device.index != torch.cuda.current_device():
            with torch.cuda.device(self._device):
                self._launch(n)
        else:
            self._launch(n)

    # ---- host side --------------------------------------------------------------------------------------------------------------
    def _launch(self, n):
        ptr = _lib.ptr
        _lib.checked().gfn_train_step(ptr(self._tensor_table), n, ptr(self._chunk_table), self._n_chunks, ptr(self._dev_state), self.max_norm,
                                      self.growth_factor, self.backoff_factor, self.growth_interval, int(self.zero_grads),
                                      ptr(self._stats), ptr(self._ws), self._ws.numel() * 4, _lib.stream_ptr(self._device))

    def _check_param(self, p):
        if not p.is_cuda:
            raise _lib.GfnError("FusedAdamWStep needs parameters on an AMD GPU (torch device 'cuda'); there is no CPU path")
        if p.dtype != torch.float32:
            raise _lib.GfnError(f"FusedAdamWStep: fp32 parameters only, got {p.dtype} (fp16 / bf16 parameters are out of scope)")
        if p.is_sparse or not p.is_contiguous():
            raise _lib.GfnError(f"FusedAdamWStep: a parameter of shape {tuple(p.shape)} is not dense and contiguous")
        if self._device is None:
            self._device = p.device
        elif p.device != self._device:
            raise _lib.GfnError(f"FusedAdamWStep: parameters on different devices: {self._device} vs {p.device}")

    def _check_grad(self, name, p):
        g = p.grad
        if g.is_sparse:
            raise _lib.GfnError(f"FusedAdamWStep: {name} has a sparse gradient")
        if g.dtype != torch.float32 or g.device != p.device or g.numel() != p.numel():
            raise _lib.GfnError(f"FusedAdamWStep: the gradient of {name} must be fp32 on {p.device} with {p.numel()} elements, got "
                                f"{g.dtype} on {g.device} with {g.numel()}")
        if not g.is_contiguous():
            raise _lib.GfnError(f"FusedAdamWStep: the gradient of {name} is not contiguous (strides {g.stride()})")

    def _upload(self, arr):
        """a numpy array -> a device byte tensor, through a pinned tensor of its own (a copy in flight may still read an earlier one)"""
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
        host.numpy()[:] = raw
        return host.to(self._device, non_blocking=True)

    def _rebuild(self, entries, key):
        names = []
        for gi, i, p in entries:
            group = self.param_groups[gi]
            names.append(group["param_names"][i] if "param_names" in group else f"group{gi}.param{i}")
            self._check_param(p)
            self._check_grad(names[-1], p)
            st = self.state[p]
            if "exp_avg" not in st:                              # a parameter's first appearance
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            for k in ("exp_avg", "exp_avg_sq"):
                m = st[k]
                if m.dtype != torch.float32 or m.device != p.device or m.numel() != p.numel() or not m.is_contiguous():
                    raise _lib.GfnError(f"FusedAdamWStep: state '{k}' of {names[-1]} does not match its parameter")
        n = len(entries)
        t = np.zeros(n, dtype=_TENSOR_DT)
        if n:
            t["p"] = [p.data_ptr() for _, _, p in entries]
            t["g"] = [p.grad.data_ptr() for _, _, p in entries]
            t["exp_avg"] = [self.state[p]["exp_avg"].data_ptr() for _, _, p in entries]
            t["exp_avg_sq"] = [self.state[p]["exp_avg_sq"].data_ptr() for _, _, p in entries]
            t["numel"] = [p.numel() for _, _, p in entries]
        aligned = ((t["p"] | t["g"] | t["exp_avg"] | t["exp_avg_sq"]) & 15) == 0
        spans, chunks = build_tables(t["numel"], aligned)
        t["first_chunk"], t["n_chunks"], t["vec16"] = spans[:, 0], spans[:, 1], spans[:, 2]
        c = np.zeros(len(chunks), dtype=_CHUNK_DT)
        c["tensor"], c["first"], c["count"] = chunks[:, 0], chunks[:, 1], chunks[:, 2]
        self._tensors, self._n_chunks, self._names = t, len(c), names
        self._chunk_table = self._upload(c) if len(c) else None
        need = int(_lib.lib().gfn_train_step_ws_bytes(n, len(c)))
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=self._device)
        self._stats = torch.zeros(_lib.TS_STATS + n, dtype=torch.float32, device=self._device)
        s = self._stats
        self.last_stats = {"grad_norm": s[_lib.TS_STAT_GRAD_NORM], "param_norm": s[_lib.TS_STAT_PARAM_NORM],
                           "grad_scale": s[_lib.TS_STAT_GRAD_SCALE], "found_inf": s[_lib.TS_STAT_FOUND_INF],
                           "clip_coef": s[_lib.TS_STAT_CLIP_COEF], "nonfinite": s[_lib.TS_STATS:]}
        self._key = key

    def _upload_hyper(self, entries, hyper):
        t = self._tensors
        if len(entries):
            rows = np.asarray([hyper[gi] for gi, _, _ in entries], dtype=np.float64)
            t["lr"], t["wd"], t["beta1"], t["beta2"], t["eps"] = rows.T
        self._tensor_table = self._upload(t) if len(entries) else None
        self._hyper = hyper


# ---- the reference's trainer surface ----------------------------------------------------------------------------------------------
def to_cuda(batch):
    """trainer/train.py:7-11: every tensor of the batch dict moved to the GPU, in place; the dict is returned"""
    for key in list(batch):
        if isinstance(batch[key], torch.Tensor):
            batch[key] = batch[key].cuda()
    return batch


def train_step(train_batch, model, objective, stepper, **kwargs):
    """trainer/train.py:29-43 with a FusedAdamWStep for the optimizer and the grad scaler.  The gradients are zero on entry because the
    previous `stepper.step()` left them so.  Returns the model's output and the loss as a detached 0-dim device tensor (the reference's
    `.item()` is a synchronisation this function does not make); the logged scalars are in `stepper.last_stats`."""
    out = model(train_batch)
    loss = objective(out, train_batch)
    stepper.scale_loss(loss).backward()
    stepper.step()
    return {"train_out": out, "train_loss": loss.detach()}


def train_k_steps_cosine(n_0, k, dataloader, model, objective, stepper, lr_scheduler, progress_bar=False, warmup=None, ema_model=None,
                         **kwargs):
    """trainer/train.py:45-64: k steps from step number n_0 on batches drawn with next(dataloader), `model.train(True)` before every
    step, then one `lr_scheduler.step()`.  There is no progress bar and no wandb: `progress_bar`, `warmup` and `ema_model` are
    accepted, as the reference accepts them, and not used.  Returns the last step's result (None when k = 0)."""
    result = None
    for step_number in range(n_0, n_0 + k):
        model.train(True)
        result = train_step(to_cuda(next(dataloader)), model, objective, stepper, lr_scheduler=lr_scheduler, n=step_number)
    lr_scheduler.step()
    return result


def reference_step(params, grads, state, hyper):
    """One step of FusedAdamWStep restated on the CPU with torch's own pieces, in the dtype of `params` (float64 for an oracle, float32
    for a calibration run): GradScaler's unscale, `torch.nn.utils.clip_grad_norm_`, `torch.optim.AdamW(foreach=False)` and
    `_amp_update_scale_` with the floor of trainer/train.py:40-41.  No GPU call.

    params: list of tensors; grads: list of the SCALED gradients, None where a parameter has none (left out, as torch leaves it out);
    state: {"exp_avg": [tensor or None], "exp_avg_sq": [...], "step": int, "scale": float, "tracker": int};
    hyper: {"groups": [{"params": [indices], "lr", "betas", "eps", "weight_decay"}], "max_norm", "growth_factor", "backoff_factor",
            "growth_interval", "min_scale"}.
    Nothing is modified; returns (params, state, stats) after the step, stats = {"grad_norm", "param_norm", "grad_scale", "found_inf",
    "nonfinite" (indices), "clip_coef"}."""
    dtype = params[0].dtype
    n = len(params)
    have = [i for i in range(n) if grads[i] is not None]
    scale = torch.tensor(float(state["scale"]), dtype=torch.float32)            # GradScaler keeps its scale in fp32 ...
    inv = scale.double().reciprocal().float().to(dtype)                        # ... and unscale_ multiplies by this
    nonfinite = [i for i in have if not bool(torch.isfinite(grads[i]).all())]
    found_inf = bool(nonfinite)
    new_p = [p.detach().clone() for p in params]
    moments = {k: [None if t is None else t.detach().clone() for t in state[k]] for k in ("exp_avg", "exp_avg_sq")}
    unscaled = {i: grads[i].detach().to(dtype) * inv for i in have}
    zero = torch.zeros((), dtype=dtype)
    grad_norm = torch.stack([torch.linalg.vector_norm(unscaled[i]) for i in have]).norm() if have else zero      # :20-23
    param_norm = torch.stack([torch.linalg.vector_norm(new_p[i]) for i in have]).norm() if have else zero       # :16-18
    step, tracker = int(state["step"]), int(state["tracker"])
    clip_coef = min(1.0, float(hyper["max_norm"]) / (float(grad_norm) + 1e-6)) if have and not found_inf else float("nan")
    if have and not found_inf:
        leaves = {i: torch.nn.Parameter(new_p[i]) for i in have}              # shares new_p's storage
        for i in have:
            leaves[i].grad = unscaled[i].clone()
            for k in ("exp_avg", "exp_avg_sq"):
                if moments[k][i] is None:
                    moments[k][i] = torch.zeros_like(new_p[i])
        torch.nn.utils.clip_grad_norm_([leaves[i] for i in have], float(hyper["max_norm"]), foreach=False)
        groups = []
        for g in hyper["groups"]:
            members = [leaves[i] for i in g["params"] if i in leaves]
            if members:
                groups.append({"params": members, "lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"]})
        opt = torch.optim.AdamW(groups, foreach=False, amsgrad=False, maximize=False)
        for i in have:     # one shared step count: the device step of FusedAdamWStep
            opt.state[leaves[i]] = {"step": torch.tensor(float(step)), "exp_avg": moments["exp_avg"][i], "exp_avg_sq": moments["exp_avg_sq"][i]}
        opt.step()
        step += 1
    # torch/amp/grad_scaler.py, _amp_update_scale_ (in fp32), then the floor
    if found_inf:
        scale, tracker = scale * float(hyper["backoff_factor"]), 0
    else:
        tracker += 1
        if tracker == int(hyper["growth_interval"]):
            grown = scale * float(hyper["growth_factor"])
            if bool(torch.isfinite(grown)):
                scale = grown
            tracker = 0
    new_scale = max(float(scale), float(torch.tensor(float(hyper["min_scale"]), dtype=torch.float32)))
    new_state = {"exp_avg": moments["exp_avg"], "exp_avg_sq": moments["exp_avg_sq"], "step": step, "scale": new_scale, "tracker": tracker}
    stats = {"grad_norm": grad_norm, "param_norm": param_norm, "grad_scale": float(state["scale"]), "found_inf": found_inf,
             "nonfinite": nonfinite, "clip_coef": clip_coef}
    return [p.detach() for p in new_p], new_state, stats
