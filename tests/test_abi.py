"""CPU: the C-ABI library builds, loads and exports every symbol include/gnn_spmm.h declares;
host-side configuration logic (no kernel launches — there is no GPU here)."""
import ctypes
import os
import re

import pytest

from gnn_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(headers=("gnn_spmm.h", "gnn_layers.h", "gnn_optim.h", "gnn_extract.h", "gnn_step.h", "gnn_stage.h")):
    txt = ""
    for h in headers:
        with open(os.path.join(REPO, "include", h)) as f:
            txt += f.read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gnn_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_header_symbols():
    L = _lib.lib()
    decl = _declared()
    assert len(decl) >= 12
    for name in decl:
        assert hasattr(L, name), f"{name} declared in gnn_spmm.h but not exported"
    assert set(decl) == set(_lib.EXPORTED_SYMBOLS)


def test_sampler_library_exports_header_symbols():
    L = _lib.sampler_lib()
    decl = _declared(("gnn_sampler.h",))
    for name in decl:
        assert hasattr(L, name), f"{name} declared in gnn_sampler.h but not exported"
    assert set(decl) == set(_lib.SAMPLER_EXPORTED_SYMBOLS)


def test_host_gather_rows():
    import numpy as np

    L = _lib.sampler_lib()
    src = np.arange(50 * 7, dtype=np.float32).reshape(50, 7)
    idx = np.array([3, 0, 49, 3], np.int64)
    dst = np.full((4, 8), -1.0, np.float32)
    _lib.check_sampler(L.gnn_host_gather_rows_f32(src.ctypes.data, 7, 50, idx.ctypes.data, 4, 7, dst.ctypes.data, 8),
                       "gather")
    assert np.array_equal(dst[:, :7], src[idx]) and np.all(dst[:, 7] == 0)
    bad = np.array([50], np.int64)
    assert L.gnn_host_gather_rows_f32(src.ctypes.data, 7, 50, bad.ctypes.data, 1, 7, dst.ctypes.data, 8) != 0


def test_version_and_error_strings():
    L = _lib.lib()
    assert b"gfx950" in L.gnn_version()
    assert L.gnn_last_error() is not None


def test_argument_validation_without_gpu():
    L = _lib.lib()
    # negative sizes are rejected before any HIP call
    rc = L.gnn_spmm_csr_f32(None, None, None, -1, 1, 1, None, 1, None, 1, 1, None, 0, 0, None)
    assert rc == -22 and b"negative" in L.gnn_last_error()
    with pytest.raises(RuntimeError, match="negative size"):
        _lib.check(L.gnn_gather_rows_f32(None, 1, None, None, 1, None, -5, 1, None), "gather")
    with pytest.raises(RuntimeError, match="negative size"):
        _lib.check(L.gnn_gather_rows_host_f32(None, 1, None, None, 1, None, -5, 1, None), "gather_host")
    assert L.gnn_gather_rows_host_f32(None, 8, None, None, 8, None, 0, 8, None) == 0  # empty: no-op
    assert L.gnn_host_register(None, 0) == -22 and b"NULL" in L.gnn_last_error()
    # F larger than the row stride
    rc = L.gnn_spmm_csr_f32(None, None, None, 4, 4, 0, None, 2, None, 8, 4, None, 0, 0, None)
    assert rc == -22 and b"ldx" in L.gnn_last_error()
    # zero-size problems are no-ops (nothing launched)
    assert L.gnn_spmm_csr_f32(None, None, None, 0, 4, 0, None, 8, None, 8, 8, None, 0, 0, None) == 0


# ---- refusals of the aggregation entry points ----------------------------------------------------
# Every call below is refused (or returns early) on the host, before the first HIP call, so the
# pointers are never read: _P stands for "some 16-byte aligned address", _BIG for "a workspace large
# enough". The default shape is a 4-row operand over K = 64 with 57 entries and unit_nnz = 16 (the
# unit kernel, 4 units, so the workspace is needed).
_P = 0x10000
_BIG = 1 << 40
_CSR = dict(rowptr=_P, col=_P, val=_P, M=4, K=64, nnz=57, X=_P, ldx=12, Y=_P, ldy=12, F=12, ws=_P, wsb=_BIG, unit=16)
_BLOCK = dict(indptr=_P, indices=_P, degree=_P, N=64, nnz=57, X=_P, ldx=12, kind=0, Y=_P, ldy=12, F=12, ws=_P,
              wsb=_BIG)


def _call_csr_f32(L, **kw):
    a = dict(_CSR, **kw)
    return L.gnn_spmm_csr_f32(a["rowptr"], a["col"], a["val"], a["M"], a["K"], a["nnz"], a["X"], a["ldx"], a["Y"],
                              a["ldy"], a["F"], a["ws"], a["wsb"], a["unit"], None)


def _call_csr_f32_ex(L, **kw):
    a = dict(_CSR, R=None, ldr=0, rmap=None)
    a.update(kw)
    return L.gnn_spmm_csr_f32_ex(a["rowptr"], a["col"], a["val"], a["M"], a["K"], a["nnz"], a["X"], a["ldx"], a["Y"],
                                 a["ldy"], a["F"], a["R"], a["ldr"], a["rmap"], a["ws"], a["wsb"], a["unit"], None)


def _call_csr_h16_f32(L, **kw):
    a = dict(_CSR, ldx=8, ldy=8, F=8, kind=1)
    a.update(kw)
    return L.gnn_spmm_csr_h16_f32(a["rowptr"], a["col"], a["val"], a["M"], a["K"], a["nnz"], a["X"], a["ldx"],
                                  a["kind"], a["Y"], a["ldy"], a["F"], a["ws"], a["wsb"], a["unit"], None)


def _call_graph_f32(L, **kw):
    a = dict(_BLOCK, row0=0, rows=4, e0=0)
    a.update(kw)
    return L.gnn_spmm_graph_f32(a["indptr"], a["indices"], a["degree"], a["N"], a["row0"], a["rows"], a["e0"],
                                a["nnz"], a["X"], a["ldx"], a["kind"], a["Y"], a["ldy"], a["F"], a["ws"], a["wsb"], None)


def _call_rows_f32(L, **kw):
    a = dict(_BLOCK, rows=_P, M=4, rowseg=_P, table=_P, K=64)
    a.update(kw)
    return L.gnn_spmm_rows_f32(a["indptr"], a["indices"], a["degree"], a["N"], a["rows"], a["M"], a["rowseg"],
                               a["nnz"], a["table"], a["K"], a["X"], a["ldx"], a["kind"], a["Y"], a["ldy"], a["F"],
                               a["ws"], a["wsb"], None, None)


_H16 = dict(kind=1, F=8, ldx=8, ldy=8)  # a 16-bit call of the block entry points

# (call, arguments that differ from the defaults, the entry point the message names, its distinguishing words)
_REFUSED = [
    # gnn_spmm_csr_f32 (a wrapper of _ex: its messages say gnn_spmm_csr_f32)
    (_call_csr_f32, dict(M=-1), "gnn_spmm_csr_f32", "negative"),
    (_call_csr_f32, dict(F=-1), "gnn_spmm_csr_f32", "negative"),
    (_call_csr_f32, dict(M=1 << 31), "gnn_spmm_csr_f32", "2^31"),
    (_call_csr_f32, dict(nnz=1 << 31), "gnn_spmm_csr_f32", "2^31"),
    (_call_csr_f32, dict(ldx=8), "gnn_spmm_csr_f32", "F (12) > ldx (8)"),
    (_call_csr_f32, dict(ldy=8), "gnn_spmm_csr_f32", "F (12) > ldy (8)"),
    (_call_csr_f32, dict(rowptr=None), "gnn_spmm_csr_f32", "NULL rowptr/Y"),
    (_call_csr_f32, dict(Y=None), "gnn_spmm_csr_f32", "NULL rowptr/Y"),
    (_call_csr_f32, dict(col=None), "gnn_spmm_csr_f32", "NULL col/val/X"),
    (_call_csr_f32, dict(X=None), "gnn_spmm_csr_f32", "NULL col/val/X"),
    (_call_csr_f32, dict(ws=None), "gnn_spmm_csr_f32", "workspace too small (%d < 512)" % _BIG),
    (_call_csr_f32, dict(wsb=511), "gnn_spmm_csr_f32", "workspace too small (511 < 512)"),
    (_call_csr_f32, dict(ws=_P + 8), "gnn_spmm_csr_f32", "workspace not 16-byte aligned"),
    # two failing conditions: the earlier check speaks
    (_call_csr_f32, dict(M=-1, ldx=8), "gnn_spmm_csr_f32", "negative"),
    (_call_csr_f32, dict(M=1 << 31, ldx=8), "gnn_spmm_csr_f32", "2^31"),
    (_call_csr_f32, dict(ldx=8, ldy=8), "gnn_spmm_csr_f32", "> ldx"),
    (_call_csr_f32, dict(ldy=8, Y=None), "gnn_spmm_csr_f32", "> ldy"),
    (_call_csr_f32, dict(rowptr=None, X=None), "gnn_spmm_csr_f32", "NULL rowptr/Y"),
    (_call_csr_f32, dict(X=None, ws=None), "gnn_spmm_csr_f32", "NULL col/val/X"),
    (_call_csr_f32, dict(ws=_P + 8, wsb=0), "gnn_spmm_csr_f32", "workspace too small"),
    # gnn_spmm_csr_f32_ex: the shared checks say gnn_spmm_csr_f32, the residual's own say _ex
    (_call_csr_f32_ex, dict(K=-1), "gnn_spmm_csr_f32", "negative"),
    (_call_csr_f32_ex, dict(K=1 << 31), "gnn_spmm_csr_f32", "2^31"),
    (_call_csr_f32_ex, dict(ldx=8), "gnn_spmm_csr_f32", "F (12) > ldx (8)"),
    (_call_csr_f32_ex, dict(ldy=8), "gnn_spmm_csr_f32", "F (12) > ldy (8)"),
    (_call_csr_f32_ex, dict(val=None), "gnn_spmm_csr_f32", "NULL col/val/X"),
    (_call_csr_f32_ex, dict(rmap=_P), "gnn_spmm_csr_f32_ex", "rmap needs R"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P, ldr=8), "gnn_spmm_csr_f32_ex", "rmap needs R"),
    (_call_csr_f32_ex, dict(rmap=_P, X=None), "gnn_spmm_csr_f32", "NULL col/val/X"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P, ldr=12, wsb=8), "gnn_spmm_csr_f32", "workspace too small (8 < 512)"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P, ldr=12, ws=_P + 4), "gnn_spmm_csr_f32", "workspace not 16-byte aligned"),
    # the residual's alignment for the vector width of the call (4 here): unit kernel, then row kernel
    (_call_csr_f32_ex, dict(rmap=_P, R=_P + 4, ldr=12), "gnn_spmm_csr_f32_ex", "R (ldr 12) not aligned for 4-wide"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P, ldr=14), "gnn_spmm_csr_f32_ex", "R (ldr 14) not aligned for 4-wide"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P + 4, ldr=12, ws=None), "gnn_spmm_csr_f32", "workspace too small"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P + 8, ldr=12, nnz=4, unit=0, ws=None), "gnn_spmm_csr_f32_ex",
     "R (ldr 12) not aligned for 4-wide"),
    (_call_csr_f32_ex, dict(rmap=_P, R=_P + 4, ldr=14, ldx=14, ldy=14, F=14, nnz=4, unit=0), "gnn_spmm_csr_f32_ex",
     "R (ldr 14) not aligned for 2-wide"),
    # gnn_spmm_csr_h16_f32
    (_call_csr_h16_f32, dict(kind=0), "gnn_spmm_csr_h16_f32", "kind 0 is neither"),
    (_call_csr_h16_f32, dict(kind=3), "gnn_spmm_csr_h16_f32", "kind 3 is neither"),
    (_call_csr_h16_f32, dict(nnz=-1), "gnn_spmm_csr_h16_f32", "negative"),
    (_call_csr_h16_f32, dict(K=1 << 31), "gnn_spmm_csr_h16_f32", "2^31"),
    (_call_csr_h16_f32, dict(ldx=4), "gnn_spmm_csr_h16_f32", "F (8) > ldx (4)"),
    (_call_csr_h16_f32, dict(ldx=4, K=0, nnz=0), "gnn_spmm_csr_h16_f32", "F (8) > ldx (4)"),  # no K == 0 exemption
    (_call_csr_h16_f32, dict(ldy=4), "gnn_spmm_csr_h16_f32", "F (8) > ldy (4)"),
    (_call_csr_h16_f32, dict(ldy=4, M=0), "gnn_spmm_csr_h16_f32", "F (8) > ldy (4)"),  # no M == 0 exemption
    (_call_csr_h16_f32, dict(F=6), "gnn_spmm_csr_h16_f32", "must be multiples of 4"),
    (_call_csr_h16_f32, dict(ldx=10), "gnn_spmm_csr_h16_f32", "must be multiples of 4"),
    (_call_csr_h16_f32, dict(ldy=10), "gnn_spmm_csr_h16_f32", "must be multiples of 4"),
    (_call_csr_h16_f32, dict(X=_P + 4), "gnn_spmm_csr_h16_f32", "X not 8-byte aligned"),
    (_call_csr_h16_f32, dict(Y=_P + 8), "gnn_spmm_csr_h16_f32", "Y not 16-byte aligned"),
    (_call_csr_h16_f32, dict(Y=_P + 8, M=0), "gnn_spmm_csr_h16_f32", "Y not 16-byte aligned"),  # before the early return
    (_call_csr_h16_f32, dict(rowptr=None), "gnn_spmm_csr_h16_f32", "NULL rowptr/Y"),
    (_call_csr_h16_f32, dict(X=None), "gnn_spmm_csr_h16_f32", "NULL col/val/X"),
    (_call_csr_h16_f32, dict(ws=None), "gnn_spmm_csr_h16_f32", "workspace too small (%d < 256)" % _BIG),
    (_call_csr_h16_f32, dict(wsb=255), "gnn_spmm_csr_h16_f32", "workspace too small (255 < 256)"),
    (_call_csr_h16_f32, dict(ws=_P + 8), "gnn_spmm_csr_h16_f32", "workspace not 16-byte aligned"),
    (_call_csr_h16_f32, dict(kind=0, M=-1), "gnn_spmm_csr_h16_f32", "kind 0 is neither"),
    (_call_csr_h16_f32, dict(M=-1, ldx=4), "gnn_spmm_csr_h16_f32", "negative"),
    (_call_csr_h16_f32, dict(ldx=4, ldy=4), "gnn_spmm_csr_h16_f32", "> ldx"),
    (_call_csr_h16_f32, dict(F=6, X=_P + 4), "gnn_spmm_csr_h16_f32", "must be multiples of 4"),
    (_call_csr_h16_f32, dict(X=_P + 4, Y=_P + 8), "gnn_spmm_csr_h16_f32", "X not 8-byte aligned"),
    (_call_csr_h16_f32, dict(Y=_P + 8, rowptr=None), "gnn_spmm_csr_h16_f32", "Y not 16-byte aligned"),
    # gnn_spmm_graph_f32
    (_call_graph_f32, dict(kind=3), "gnn_spmm_graph_f32", "kind 3 is none of"),
    (_call_graph_f32, dict(rows=-1), "gnn_spmm_graph_f32", "negative"),
    (_call_graph_f32, dict(e0=-1), "gnn_spmm_graph_f32", "negative"),
    (_call_graph_f32, dict(rows=1 << 31), "gnn_spmm_graph_f32", "2^31"),
    (_call_graph_f32, dict(N=1 << 31), "gnn_spmm_graph_f32", "2^31"),
    (_call_graph_f32, dict(row0=61), "gnn_spmm_graph_f32", "row0 (61) + rows (4) > num_nodes (64)"),
    (_call_graph_f32, dict(ldx=8), "gnn_spmm_graph_f32", "F (12) > ldx (8)"),
    (_call_graph_f32, dict(ldy=8), "gnn_spmm_graph_f32", "F (12) > ldy (8)"),
    (_call_graph_f32, dict(_H16, F=6), "gnn_spmm_graph_f32", "must be multiples of 4"),
    (_call_graph_f32, dict(_H16, kind=2, ldx=10), "gnn_spmm_graph_f32", "must be multiples of 4"),
    (_call_graph_f32, dict(_H16, X=_P + 4), "gnn_spmm_graph_f32", "X not 8-byte aligned"),
    (_call_graph_f32, dict(_H16, Y=_P + 8), "gnn_spmm_graph_f32", "Y not 16-byte aligned"),
    (_call_graph_f32, dict(ws=None), "gnn_spmm_graph_f32", "workspace too small (0 < "),
    (_call_graph_f32, dict(wsb=4096), "gnn_spmm_graph_f32", "workspace too small (4096 < "),
    (_call_graph_f32, dict(ws=_P + 8), "gnn_spmm_graph_f32", "workspace not 16-byte aligned"),
    (_call_graph_f32, dict(indptr=None), "gnn_spmm_graph_f32", "NULL indptr/degree/Y"),
    (_call_graph_f32, dict(Y=None), "gnn_spmm_graph_f32", "NULL indptr/degree/Y"),
    (_call_graph_f32, dict(indices=None), "gnn_spmm_graph_f32", "NULL indices/X"),
    (_call_graph_f32, dict(X=None), "gnn_spmm_graph_f32", "NULL indices/X"),
    (_call_graph_f32, dict(kind=3, rows=-1), "gnn_spmm_graph_f32", "kind 3 is none of"),
    (_call_graph_f32, dict(rows=-1, ldx=8), "gnn_spmm_graph_f32", "negative"),
    (_call_graph_f32, dict(row0=61, ldx=8), "gnn_spmm_graph_f32", "> num_nodes"),
    (_call_graph_f32, dict(ldx=8, ldy=8), "gnn_spmm_graph_f32", "> ldx"),
    (_call_graph_f32, dict(_H16, ldy=4, Y=_P + 8), "gnn_spmm_graph_f32", "> ldy"),
    (_call_graph_f32, dict(_H16, Y=_P + 8, ws=None), "gnn_spmm_graph_f32", "Y not 16-byte aligned"),
    (_call_graph_f32, dict(ws=None, indptr=None), "gnn_spmm_graph_f32", "workspace too small"),
    (_call_graph_f32, dict(ws=None, rows=0), "gnn_spmm_graph_f32", "workspace too small"),  # before the early return
    # gnn_spmm_rows_f32
    (_call_rows_f32, dict(kind=-1), "gnn_spmm_rows_f32", "kind -1 is none of"),
    (_call_rows_f32, dict(M=-1), "gnn_spmm_rows_f32", "negative"),
    (_call_rows_f32, dict(K=-1), "gnn_spmm_rows_f32", "negative"),
    (_call_rows_f32, dict(M=1 << 31), "gnn_spmm_rows_f32", "2^31"),
    (_call_rows_f32, dict(nnz=1 << 31), "gnn_spmm_rows_f32", "2^31"),
    (_call_rows_f32, dict(K=65), "gnn_spmm_rows_f32", "K (65) > num_nodes (64)"),
    (_call_rows_f32, dict(ldx=8), "gnn_spmm_rows_f32", "F (12) > ldx (8)"),
    (_call_rows_f32, dict(ldy=8), "gnn_spmm_rows_f32", "F (12) > ldy (8)"),
    (_call_rows_f32, dict(_H16, F=6), "gnn_spmm_rows_f32", "must be multiples of 4"),
    (_call_rows_f32, dict(_H16, kind=2, ldy=10), "gnn_spmm_rows_f32", "must be multiples of 4"),
    (_call_rows_f32, dict(_H16, X=_P + 4), "gnn_spmm_rows_f32", "X not 8-byte aligned"),
    (_call_rows_f32, dict(_H16, Y=_P + 8), "gnn_spmm_rows_f32", "Y not 16-byte aligned"),
    (_call_rows_f32, dict(ws=None), "gnn_spmm_rows_f32", "workspace too small (0 < "),
    (_call_rows_f32, dict(wsb=1024), "gnn_spmm_rows_f32", "workspace too small (1024 < "),
    (_call_rows_f32, dict(ws=_P + 8), "gnn_spmm_rows_f32", "workspace not 16-byte aligned"),
    (_call_rows_f32, dict(rowseg=None), "gnn_spmm_rows_f32", "NULL indptr/degree/rows/rowseg/Y"),
    (_call_rows_f32, dict(table=None), "gnn_spmm_rows_f32", "NULL or misaligned table"),
    (_call_rows_f32, dict(table=_P + 4), "gnn_spmm_rows_f32", "NULL or misaligned table"),
    (_call_rows_f32, dict(indices=None), "gnn_spmm_rows_f32", "NULL indices/X"),
    (_call_rows_f32, dict(X=None), "gnn_spmm_rows_f32", "NULL indices/X"),
    (_call_rows_f32, dict(kind=-1, M=-1), "gnn_spmm_rows_f32", "kind -1 is none of"),
    (_call_rows_f32, dict(M=1 << 31, K=65), "gnn_spmm_rows_f32", "2^31"),
    (_call_rows_f32, dict(K=65, ldx=8), "gnn_spmm_rows_f32", "> num_nodes"),
    (_call_rows_f32, dict(ldx=8, ldy=8), "gnn_spmm_rows_f32", "> ldx"),
    (_call_rows_f32, dict(_H16, X=_P + 4, Y=_P + 8), "gnn_spmm_rows_f32", "X not 8-byte aligned"),
    (_call_rows_f32, dict(ws=_P + 8, wsb=0), "gnn_spmm_rows_f32", "workspace too small"),
    (_call_rows_f32, dict(rowseg=None, table=None), "gnn_spmm_rows_f32", "NULL indptr/degree/rows/rowseg/Y"),
    (_call_rows_f32, dict(table=None, X=None), "gnn_spmm_rows_f32", "NULL or misaligned table"),
]

_NONE = dict(rowptr=None, col=None, val=None, X=None, Y=None, ws=None, wsb=0)
_NONE_BLOCK = dict(indptr=None, indices=None, degree=None, X=None, Y=None)  # the workspace is checked first
# calls that return 0 before the NULL checks: an empty output (M == 0 or F == 0)
_EMPTY = [
    (_call_csr_f32, dict(_NONE, M=0)),
    (_call_csr_f32, dict(_NONE, F=0)),
    (_call_csr_f32, dict(_NONE, M=0, ldy=0)),  # F <= ldy is not asked of an empty output
    (_call_csr_f32, dict(_NONE, K=0, nnz=0, ldx=0, M=0)),  # nor F <= ldx of an empty X
    (_call_csr_f32_ex, dict(_NONE, M=0, rmap=_P)),  # before the residual's checks too
    (_call_csr_f32_ex, dict(_NONE, F=0)),
    (_call_csr_h16_f32, dict(_NONE, M=0)),
    (_call_csr_h16_f32, dict(_NONE, F=0)),
    (_call_graph_f32, dict(_NONE_BLOCK, rows=0, nnz=0)),
    (_call_graph_f32, dict(_NONE_BLOCK, F=0)),
    (_call_graph_f32, dict(_NONE_BLOCK, rows=0, nnz=0, **_H16)),
    (_call_rows_f32, dict(_NONE_BLOCK, rows=None, rowseg=None, table=None, M=0, nnz=0)),
    (_call_rows_f32, dict(_NONE_BLOCK, rows=None, rowseg=None, table=None, F=0)),
    (_call_rows_f32, dict(_NONE_BLOCK, rows=None, rowseg=None, table=None, M=0, nnz=0, **_H16)),
]


def _spmm_env_cleared(monkeypatch):
    for k in ("GNN_SPMM_ROWK", "GNN_SPMM_ROWK_WPR", "GNN_SPMM_G", "GNN_SPMM_NJ", "GNN_SPMM_VW", "GNN_SPMM_XCD",
              "GNN_SPMM_SMALL_U16", "GNN_SPMM_CROWS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("call,args,name,words", _REFUSED,
                         ids=["%s-%d" % (c[0].__name__[6:], i) for i, c in enumerate(_REFUSED)])
def test_spmm_refusals(monkeypatch, call, args, name, words):
    """Each aggregation entry point refuses a bad call with -22 and a message that opens with the entry
    point's name and holds the words of the failed check; of two failed checks the earlier one speaks."""
    _spmm_env_cleared(monkeypatch)
    L = _lib.lib()
    L.gnn_gather_rows_f32(None, 1, None, None, 1, None, -5, 1, None)  # some other message first
    assert call(L, **args) == -22
    msg = L.gnn_last_error().decode()
    assert msg.startswith(name + ": "), msg
    assert words in msg, msg


@pytest.mark.parametrize("call,args", _EMPTY, ids=["%s-%d" % (c[0].__name__[6:], i) for i, c in enumerate(_EMPTY)])
def test_spmm_empty_calls_return_before_null_checks(monkeypatch, call, args):
    _spmm_env_cleared(monkeypatch)
    assert call(_lib.lib(), **args) == 0


def test_workspace_and_config():
    from gnn_amd.custom_sparse_ops import spmm_config

    L = _lib.lib()
    assert L.gnn_spmm_default_unit_nnz(15809, 1810000, 602) >= 16
    # very sparse rows (the layer-2 backward operand): ~2 rows per unit, never below 4
    assert L.gnn_spmm_default_unit_nnz(8680, 14876, 1024) == 4
    assert L.gnn_spmm_default_unit_nnz(1000, 100, 64) == 4
    ws = L.gnn_spmm_workspace_bytes(15809, 1810000, 602, 0)
    unit = L.gnn_spmm_default_unit_nnz(15809, 1810000, 602)
    assert ws >= ((1810000 + unit - 1) // unit) * 2 * 604 * 4
    c = spmm_config(15809, 1810000, 602)
    assert c["vw"] == 2 and c["g"] * c["nj"] * c["vw"] * c["tiles"] >= 602
    c = spmm_config(8689, 850000, 1024)
    assert c["vw"] == 4 and c["g"] * c["nj"] * 4 * c["tiles"] == 1024
    c = spmm_config(100, 1000, 602, ldx=608)
    assert c["vw"] == 2  # F itself is not a multiple of 4
    c = spmm_config(100, 1000, 5000)
    assert c["tiles"] >= 2 and c["nj"] <= 8
    # L2-sized column tiles when X rows are re-read (nnz >= 8 K): slice of X ~ 4 MiB
    c = spmm_config(8680, 868338, 1024, K=15768)  # layer-1 forward: 64-float slices
    assert (c["vw"], c["g"], c["nj"], c["tiles"]) == (4, 16, 1, 16)
    c = spmm_config(15768, 868338, 1024, K=8680)  # layer-1 backward: 128-float slices
    assert (c["vw"], c["g"], c["nj"], c["tiles"]) == (4, 32, 1, 8)
    c = spmm_config(15768, 1821171, 604, K=22153, ldx=604, ldy=604)  # layer 0, padded rows
    assert (c["vw"], c["g"], c["nj"], c["tiles"]) == (4, 16, 1, 10)
    c = spmm_config(512, 14876, 1024, K=8680)  # small operand: 256-float tiles, rows left whole
    assert (c["vw"], c["g"], c["nj"], c["tiles"]) == (4, 64, 1, 4)
    assert L.gnn_spmm_default_unit_nnz(512, 14876, 1024) == 30  # 2048 waves over 4 tiles
    # the main kernel each call launches: the layer-2 calls (<= 64 k nonzeros) take the row kernel
    # (a workgroup per (row, slice), no combine), the big layers the unit kernel; a fixed unit
    # size always asks for the unit kernel
    # long rows: the unit kernel, 256-float tiles, 16 nonzeros in flight per lane
    assert spmm_config(512, 14876, 1024, K=8680)["kernel"] == "spmm_unit_kernel<4, 64, 1, 16, false>"
    assert spmm_config(8680, 14876, 1024, K=512)["kernel"] == "spmm_row_kernel<4, 4, 4, 1, false>"
    assert spmm_config(8680, 14876, 1024, K=512, unit_nnz=4)["kernel"].startswith("spmm_unit_kernel<4, 64, 4")
    assert spmm_config(15768, 1821171, 604, K=22153, ldx=604, ldy=604)["kernel"] == \
        "spmm_unit_kernel<4, 16, 1, 4, false>"
    assert spmm_config(100, 1000, 602, ldx=608)["kernel"] == "spmm_row_kernel<2, 1, 16, 1, false>"
    assert spmm_config(100, 2000, 602, ldx=608)["kernel"].startswith("spmm_unit_kernel")  # 20 per row
    assert L.gnn_csr_transpose_workspace_bytes(10, 1000, 50) >= 4000
    assert L.gnn_segsort_workspace_bytes(100) >= 800


def _sage_config(M, D, agg=0):
    s, nv, grid = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().gnn_sage_norm_config(M, D, agg, ctypes.byref(s), ctypes.byref(nv), ctypes.byref(grid)) == 0
    return s.value, nv.value, grid.value


def test_sage_norm_config(monkeypatch):
    """The layer tail's backward dispatch (sage.hip): which form, how many float4 per lane and which grid a
    shape gets, by default and under each environment override; the workspace query covers every grid."""
    L = _lib.lib()
    for k in ("GNN_SAGE_BWD1", "GNN_SAGE_BWD_GRID", "GNN_SAGE_BWD2_GRID", "GNN_SAGE_BWD2_GRID_AGG"):
        monkeypatch.delenv(k, raising=False)
    one_wave = {4: 1, 100: 1, 256: 1, 260: 2, 508: 2, 516: 3, 1020: 4, 1028: 5, 1284: 6, 1540: 7, 2044: 8}
    split = {512: 1, 520: 2, 1024: 2, 1032: 3, 1536: 3, 1544: 4, 2048: 4}
    for agg in (0, 1):
        for D, nv in one_wave.items():  # D % 8 != 0 or D < 512: one wave per row, NV = ceil(D / 256)
            assert _sage_config(9, D, agg) == (0, nv, 3), D
            assert _sage_config(3100, D, agg) == (0, nv, 768), D  # capped at 768 workgroups of 4 rows
            assert _sage_config(3072, D, agg) == (0, nv, 768) and _sage_config(3068, D, agg) == (0, nv, 767)
        for D, nvh in split.items():  # two waves per row, NVH = ceil(D / 2 / 256)
            assert _sage_config(9, D, agg) == (1, nvh, 5), D
            assert _sage_config(4100, D, agg) == (1, nvh, 1024), D  # capped at 1,024 workgroups of 2 rows
            assert _sage_config(2046, D, agg) == (1, nvh, 1023), D
        assert _sage_config(0, 1024, agg) == (1, 2, 1) and _sage_config(0, 100, agg) == (0, 1, 1)
    # the split grid's overrides are read per call, one for each entry
    monkeypatch.setenv("GNN_SAGE_BWD2_GRID", "3")
    assert _sage_config(13, 1032, 0) == (1, 3, 3) and _sage_config(13, 1032, 1) == (1, 3, 7)
    assert _sage_config(13, 1028, 0) == (0, 5, 4)  # not the one-wave form's
    monkeypatch.setenv("GNN_SAGE_BWD2_GRID_AGG", "2048")
    assert _sage_config(4100, 1024, 1) == (1, 2, 2048) and _sage_config(4100, 1024, 0) == (1, 2, 3)
    monkeypatch.setenv("GNN_SAGE_BWD2_GRID", "2049")  # out of range: the default
    assert _sage_config(4100, 1024, 0) == (1, 2, 1024)
    for M, D in ((4100, 1024), (9, 512), (100000, 2048), (3100, 2044), (3100, 100)):
        assert L.gnn_sage_norm_bwd_workspace_bytes(M, D) >= max(_sage_config(M, D, a)[2] for a in (0, 1)) * 3 * D * 4
    # GNN_SAGE_BWD1 forces the one-wave form on the split widths
    monkeypatch.setenv("GNN_SAGE_BWD1", "1")
    for D, nv in ((512, 2), (1024, 4), (2048, 8)):
        assert _sage_config(9, D) == (0, nv, 3) and _sage_config(4100, D, 1) == (0, nv, 768)
        assert L.gnn_sage_norm_bwd_workspace_bytes(4100, D) >= 768 * 3 * D * 4
    # refused widths; output pointers are optional
    for D in (2052, 6, 0, -4):
        assert L.gnn_sage_norm_config(9, D, 0, None, None, None) != 0
        assert b"gnn_sage_norm_config" in L.gnn_last_error()
    assert L.gnn_sage_norm_config(-1, 100, 0, None, None, None) != 0
    assert L.gnn_sage_norm_config(9, 100, 0, None, None, None) == 0


_GEMM_WS_SHAPES = [(512, 602, 15809, 2), (512, 1024, 8689, 2), (15809, 512, 602, 2), (8689, 512, 1024, 2),
                   (8689, 1024, 512, 2), (101, 131, 3001, 1), (1, 5, 3, 1)]
# per shape: (gnn_gemm_f32_, gnn_gemm_f32_split3_, gnn_gemm_p3_)workspace_bytes, recorded from the library
# before the split3 kernels were folded into one template (the query is a pure function of the shape,
# the batch count and GNN_GEMM_WIDE / GNN_GEMM_SPLITS; GNN_GEMM_TAIL does not change it)
_GEMM_WS_DEFAULT = [(29589504, 46850048, 46850048), (33554432, 50331648, 50331648), (0, 0, 0),
                    (0, 8388608, 8388608), (0, 0, 0), (582164, 582164, 582164), (0, 0, 0)]
_GEMM_WS_WIDE1 = [(29589504, 51781632, 51781632), (33554432, 67108864, 67108864), (0, 0, 0), (0, 0, 0), (0, 0, 0),
                  (582164, 582164, 582164), (0, 0, 0)]


@pytest.mark.parametrize("env,expected", [({}, _GEMM_WS_DEFAULT), ({"GNN_GEMM_WIDE": "1"}, _GEMM_WS_WIDE1),
                                          ({"GNN_GEMM_WIDE": "-1"}, _GEMM_WS_DEFAULT),
                                          ({"GNN_GEMM_TAIL": "0"}, _GEMM_WS_DEFAULT)])
def test_gemm_workspace_query(monkeypatch, env, expected):
    L = _lib.lib()
    for k in ("GNN_GEMM_WIDE", "GNN_GEMM_TAIL", "GNN_GEMM_SPLITS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for shape, want in zip(_GEMM_WS_SHAPES, expected):
        got = (L.gnn_gemm_f32_workspace_bytes(*shape), L.gnn_gemm_f32_split3_workspace_bytes(*shape),
               L.gnn_gemm_p3_workspace_bytes(*shape))
        assert got == want, (env, shape)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="missing"):
        _lib.lib()


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "gnn_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
