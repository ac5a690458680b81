"""gfnet_amd/_lib.py derives the ctypes binding from include/gfnet_hip.h: the parser on a small header with every declaration form
the real one uses, the real header's prototypes and constants, and the checked view of the library (no GPU: argument errors only)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

INLINE = """
/* a comment with a prototype inside: int gfn_not_this(int a); */
#ifndef X_H
#define X_H
#include <stdint.h>
#define GFN_OK 0
#define GFN_ERR_SOME (-3)     /* parenthesised negative */
#define GFN_HALF_STD 0.0625
#define GFN_TINY 1e-7
#define GFN_MASK 0x10
#define GFN_NOT_A_NUMBER (GFN_OK + 1)
#define OTHER_THING 5
typedef void *gfn_stream_t; /* hipStream_t */
typedef struct gfn_rec {
    float *p, *g;
    int64_t numel;
} gfn_rec; /* 24 bytes */
int gfn_version(void);
const char *gfn_text(void);
int gfn_arch(char *buf, int buflen);
int64_t gfn_bytes(int B, int G);
int gfn_all(const float *f0, int64_t f0_bs, const void *f1, float *out, int B, uint64_t seed, float scale, double std,
            const float *const *flows, float *const *g_flows, const gfn_rec *table, unsigned char *mask,
            const int64_t *idx, void *scratch, int64_t scratch_bytes,
            gfn_stream_t stream);
int gfn_flag(int C, int r);
#endif
"""


def test_parser_on_every_declaration_form():
    from gfnet_amd import _lib
    from gfnet_amd._lib import c_double, c_float, c_i64, c_int, c_vp

    protos, consts = _lib.parse_header(INLINE)
    assert list(protos) == ["gfn_version", "gfn_text", "gfn_arch", "gfn_bytes", "gfn_all", "gfn_flag"]  # declaration order, no comment, no struct
    assert protos["gfn_version"] == (c_int, [])
    assert protos["gfn_text"] == (ctypes.c_char_p, [])
    assert protos["gfn_arch"] == (c_int, [c_vp, c_int])
    assert protos["gfn_bytes"] == (c_i64, [c_int, c_int])
    assert protos["gfn_all"] == (c_int, [c_vp, c_i64, c_vp, c_vp, c_int, ctypes.c_uint64, c_float, c_double, c_vp, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_i64, c_vp])
    assert protos["gfn_flag"] == (c_int, [c_int, c_int])
    assert consts == {"GFN_OK": 0, "GFN_ERR_SOME": -3, "GFN_HALF_STD": 0.0625, "GFN_TINY": 1e-7, "GFN_MASK": 16}
    assert type(consts["GFN_ERR_SOME"]) is int and type(consts["GFN_HALF_STD"]) is float


@pytest.mark.parametrize("decl, named", [
    ("int gfn_bad(const float *x, size_t n, gfn_stream_t stream);", "size_t n"),        # an unknown scalar parameter
    ("int gfn_bad(unsigned flags);", "unsigned flags"),                                 # a type of one word with no name
    ("int gfn_bad(long long n);", "long long n"),
    ("unsigned gfn_bad(int a);", "unsigned"),                                           # an unknown return type
    ("float *gfn_bad(int a);", "float *"),                                              # a returned pointer other than const char *
    ("int gfn_bad(int);", "int"),                                                       # an unnamed parameter
])
def test_parser_fails_closed(decl, named):
    from gfnet_amd import _lib

    with pytest.raises(_lib.GfnError, match=r"gfn_bad: cannot bind .*'" + re.escape(named) + "'"):
        _lib.parse_header("int gfn_good(int a);\n" + decl)


def test_real_header_prototypes_and_constants():
    from gfnet_amd import _lib

    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "gfnet_hip.h"))
    assert len(_lib.PROTOTYPES) >= 60
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    defines = re.findall(r"^#define\s+(GFN_\w+)\s+(\S+)\s*$", hdr, flags=re.M)   # this test's own scan; every one of them is numeric
    assert len(defines) >= 35
    for name, text in defines:
        short = name if name in ("GFN_F32", "GFN_F16") else name[4:]
        assert getattr(_lib, short) == _lib.CONSTANTS[name] == float(text.strip("()")), name
    assert _lib.ERR_INVALID_ARG == -1 and _lib.RL_MAX_ITR == 8 and _lib.KDE_SORTED_MIN_STD == 0.0625 and _lib.CBT_NEED_ALL == 15
    assert _lib.SAMPLE_MODES == {"bilinear": 0, "nearest": 1, "bicubic": 2} and _lib.PADDING_MODES == {"zeros": 0, "border": 1, "reflection": 2}
    # the rule behind the checked view: an int-returning entry point with a stream returns a status.  The int-returning ones without
    # a stream answer on the host; a new one has to be looked at (is its value a status?) before it joins this list
    ints = {name for name, (restype, _) in _lib.PROTOTYPES.items() if restype is _lib.c_int}
    # (gfn_conv_block_route: the count of route fields it filled, 0 for a shape the entry point refuses)
    assert ints - _lib.STATUS_FUNCS == {"gfn_abi_version", "gfn_device_arch", "gfn_local_corr_plans", "gfn_kde_msplit",
                                        "gfn_conv_block_route"}
    assert len(_lib.STATUS_FUNCS) >= 45 and _lib.STATUS_FUNCS <= ints


def test_checked_view_raises_under_the_symbols_own_name():
    from gfnet_amd import _lib

    raw, chk = _lib.lib(), _lib.checked()
    assert raw.gfn_interp_bilinear_fwd(None, None, 1, 2, 2, 2, 2, None) == _lib.ERR_INVALID_ARG      # the raw view hands the code back
    key = ("cpu", None, 0, "test_abi_binding")
    _lib._scratch[key] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.GfnError) as e:
        chk.gfn_interp_bilinear_fwd(None, None, 1, 2, 2, 2, 2, None)
    assert str(e.value) == f"gfn_interp_bilinear_fwd failed (-1): {raw.gfn_last_error().decode()}" and raw.gfn_last_error()
    assert not _lib._scratch                                                                          # dropped, as check() does
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert chk.gfn_interp_bilinear_fwd(p, p, 0, 2, 2, 2, 2, None) == 0                                # an empty batch: GFN_OK, no launch
    # a non-zero flag, count or size is an answer, not an error, in both views
    assert chk.gfn_kde_msplit(1, 20000, 20000) == raw.gfn_kde_msplit(1, 20000, 20000) >= 1
    assert chk.gfn_local_corr_plans(64, 56, 56, 32, 4, _lib.GFN_F32) == raw.gfn_local_corr_plans(64, 56, 56, 32, 4, _lib.GFN_F32) in (0, 1)
    assert chk.gfn_homography_scratch_bytes(2, 100) == raw.gfn_homography_scratch_bytes(2, 100) > 0
    assert raw.gfn_local_corr_plans.restype is _lib.c_int
