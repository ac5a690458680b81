"""ctypes binding of libgfnet_hip.so, derived from its C ABI: include/gfnet_hip.h is read at import.

Every `gfn_*` prototype of the header gives the argument and return ctypes of its symbol, every `#define GFN_<NAME> <number>` a
constant of this module (`GFN_RL_STATS` -> `RL_STATS`; `GFN_F32` / `GFN_F16` keep their prefix, `GFN_BF16` has both names): nothing of the boundary is typed
a second time here.  A declaration the parser does not understand is an error at import, never a default.

torch is imported first so that the library binds to the HIP runtime torch already loaded
(same libamdhip64 SONAME); torch itself is only plumbing here: device memory and streams.
There is NO CPU fallback: if the library is missing or the tensors are not on a GPU the ops raise.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GFNET_HIP_LIB") or os.path.join(_HERE, "csrc", "libgfnet_hip.so")
HEADER_PATH = os.environ.get("GFNET_HIP_HEADER") or os.path.join(_HERE, "..", "include", "gfnet_hip.h")

c_int, c_i64, c_vp, c_float, c_double = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
_SCALARS = {"int": c_int, "int64_t": c_i64, "uint64_t": ctypes.c_uint64, "float": c_float, "double": c_double, "gfn_stream_t": c_vp}


class GfnError(RuntimeError):
    pass


def _ctype(decl, proto, is_return=False):
    """The ctypes type of one parameter declaration (type and name) or of a return type: every pointer is a c_void_p (a returned
    `const char *` a c_char_p), a scalar is looked up by its type name; anything else raises, naming the prototype."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        if not is_return:
            return c_vp
        if words == ["const", "char", "*"]:
            return ctypes.c_char_p
    kind = [w for w in (words if is_return else words[:-1]) if w != "const"]
    if len(kind) != 1 or kind[0] not in _SCALARS:
        raise GfnError(f"{proto}: cannot bind {'return type' if is_return else 'parameter'} '{' '.join(decl.split())}' "
                       f"(known: pointers, {', '.join(_SCALARS)})")
    return _SCALARS[kind[0]]


def parse_header(text):
    """(prototypes, constants) of a C header written like include/gfnet_hip.h: prototypes maps every `gfn_*` function to (restype,
    [argtypes]) in declaration order, constants every `#define GFN_<NAME> <int or float literal, possibly parenthesised>` to its
    value under the header's name."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GFN_\w+)[ \t]+\(?[ \t]*([-+]?[0-9.][\w.+-]*)[ \t]*\)?[ \t]*$", text, flags=re.M):
        try:
            constants[name] = int(value, 0)
        except ValueError:
            constants[name] = float(value)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(gfn_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() == "void" else params.split(",")
        prototypes[name] = (_ctype(ret, name, is_return=True), [_ctype(p, name) for p in params])
    return prototypes, constants


try:
    with open(HEADER_PATH) as _f:
        PROTOTYPES, CONSTANTS = parse_header(_f.read())
except OSError as e:
    raise GfnError(f"the C ABI header is needed to bind the library: {e} (set GFNET_HIP_HEADER to include/gfnet_hip.h)") from None
globals().update({name if name in ("GFN_F32", "GFN_F16") else name[len("GFN_"):]: value for name, value in CONSTANTS.items()})
GFN_BF16 = CONSTANTS["GFN_BF16"]  # beside GFN_F32 / GFN_F16; the rule above also gives it as BF16
# F.grid_sample's `mode` / `padding_mode` strings -> GFN_SAMPLE_* / GFN_PAD_*
SAMPLE_MODES = {mode: CONSTANTS["GFN_SAMPLE_" + mode.upper()] for mode in ("bilinear", "nearest", "bicubic")}
PADDING_MODES = {mode: CONSTANTS["GFN_PAD_" + mode.upper()] for mode in ("zeros", "border", "reflection")}
# The entry points whose int is a status (GFN_OK or a negative GFN_ERR_*): those that return int AND take a gfn_stream_t, i.e. that
# enqueue work.  What takes no stream answers a question on the host (sizes, gfn_local_corr_plans' flag, gfn_kde_msplit's count,
# the introspection calls) and its value is never an error code to raise on.
STATUS_FUNCS = frozenset(name for name, (restype, argtypes) in PROTOTYPES.items() if restype is c_int and argtypes[-1:] == [c_vp])

_handles = {}


def _load(checked):
    if not os.path.exists(LIB_PATH):
        raise GfnError(f"{LIB_PATH} not found: build it with `python -m gfnet_amd.build` "
                       "(there is no CPU fallback for the GFNet hot path)")
    L = ctypes.CDLL(LIB_PATH)  # (a handle of its own per view: ctypes keeps one function object per handle and name)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
        if checked and name in STATUS_FUNCS:
            fn.errcheck = _raise_on_error
    _handles[checked] = L
    return L


def lib():
    """Load (once) and return the raw ctypes handle: status codes come back as integers.  Raises if the HIP library has not been built."""
    return _handles.get(False) or _load(False)


def checked():
    """The same library with every status-returning entry point (STATUS_FUNCS) raising GfnError by itself, under the name of the
    symbol that was called; sizes, flags and counts come back as they are."""
    return _handles.get(True) or _load(True)


def exported_symbols():
    return list(PROTOTYPES)


def check(code, what):
    if code != 0:
        msg = lib().gfn_last_error().decode()
        # gfn_local_corr_fwd wants its scratch counters zero on entry and only a call that ran to the end leaves them so
        # (include/gfnet_hip.h): after any failure the cached buffers are dropped, the next call gets freshly zeroed ones
        for b in _scratch.values():
            _retire(b)  # (not freed where a captured graph may still name them)
        _scratch.clear()
        raise GfnError(f"{what} failed ({code}): {msg}")


def _raise_on_error(code, fn, args):
    if code != 0:
        check(code, fn.__name__)
    return code


def ptr(t):
    return c_vp(t.data_ptr()) if t is not None else c_vp(0)


# the current stream's raw handle: torch.cuda.current_stream() builds a Stream object per call (~4.5 us; a step makes ~150 calls and the
# three-scene workload is bound by the host's launch rate), the C hook returns the handle itself
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_handle(device):
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


def stream_ptr(device):
    return c_vp(current_stream_handle(device))


def require_gpu(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise GfnError("gfnet_amd ops need tensors on an AMD GPU (torch device 'cuda'); there is no CPU path")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise GfnError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


_scratch = {}
_retired = []  # outgrown or dropped scratch buffers that were handed out DURING a stream capture: a hipGraph still names them
_in_graphs = set()  # data_ptr of every buffer scratch() returned while its stream was capturing


def _retire(buf):
    """A buffer leaves the cache: kept alive only if a captured graph may name it (the list used to take every outgrown or
    dropped buffer, ~9 MB each at 448b32, whether or not a graph had ever been captured)."""
    if buf.data_ptr() in _in_graphs:
        _retired.append(buf)


def release_retired():
    """Free the scratch buffers kept alive for captured graphs; call after destroying those graphs."""
    _in_graphs.difference_update(b.data_ptr() for b in _retired)
    _retired.clear()


def scratch(device, nbytes, pool=""):
    """A per-(device, stream), grow-only int32 scratch buffer.  Reuse is stream-ordered: any number of models may share it on
    one stream (their launches cannot overlap), work on different streams gets different buffers; one host thread per
    stream.  Dropped as a whole after any failed call (check()).  `pool` names a buffer of its own: the default one belongs to the
    local correlation, whose counters must be zero on entry, so an op that leaves other contents behind (the loss's partial sums)
    takes another."""
    key = (device.type, device.index, current_stream_handle(device) if device.type == "cuda" else 0, pool)
    buf = _scratch.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        # a buffer that is outgrown is RETIRED, not freed: a hipGraph captured on this stream keeps launching kernels with its
        # address (round 4: two scenes of different sizes captured on one stream -- the second capture grew the buffer and the first
        # graph's replays ended in a memory fault).  A few MB per growth step, a handful of steps per process.
        if buf is not None:
            _retire(buf)
        # zero-filled: gfn_local_corr_fwd wants its counters zero on entry and leaves them zero (include/gfnet_hip.h)
        buf = torch.zeros((max(nbytes, 1 << 16) + 3) // 4, device=device, dtype=torch.int32)
        _scratch[key] = buf
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        _in_graphs.add(buf.data_ptr())
    return buf


def mode_codes(sample_mode, padding_mode, what):
    """(GFN_SAMPLE_*, GFN_PAD_*) of two F.grid_sample mode strings; ValueError naming the accepted values otherwise."""
    if sample_mode not in SAMPLE_MODES or padding_mode not in PADDING_MODES:
        raise ValueError(f"{what}: sample_mode must be one of {sorted(SAMPLE_MODES)} and padding_mode one of {sorted(PADDING_MODES)}, "
                         f"got {sample_mode!r}, {padding_mode!r}")
    return SAMPLE_MODES[sample_mode], PADDING_MODES[padding_mode]


def featc(t):
    """A feature map as the kernels read it: contiguous, fp32 or fp16 as stored (BASELINE config 5: fp16 pyramids are read
    directly, no widened copy); returns (tensor, dtype code).  Other dtypes (bf16, fp64) are widened to fp32."""
    if t.dtype == torch.float16:
        return t.contiguous(), GFN_F16
    return f32c(t), GFN_F32


def f32c(t):
    """fp32 + contiguous (no copy when already so)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
