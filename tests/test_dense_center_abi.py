"""The dense store's centre (cm_dense_set_center / cm_dense_get_center / cm_dense_mean and the fp64
sums behind it): declared in the header, exported by the library, bound with the header's argument
types, and refusing a NULL handle before any device call (CPU-only container)."""
import ctypes
import re
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "classmate_hip.h"
LIB = REPO / "classmate-rag_amd" / "classmate_hip" / "libclassmate_hip.so"

# the header's prototypes, argument by argument
PROTOS = {
    "cm_dense_set_center": "int cm_dense_set_center(cm_dense *h, const float *mu);",
    "cm_dense_get_center": "int cm_dense_get_center(cm_dense *h, float *mu_out, int32_t *is_set);",
    "cm_dense_mean": "int cm_dense_mean(cm_dense *h, float *mean_out, int64_t *n_live_out);",
    "cm_dense_column_sums": "int cm_dense_column_sums(cm_dense *h, double *sums_out, int64_t *n_live_out);",
}


def test_declared_in_the_header():
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S))
    for name, proto in PROTOS.items():
        assert proto in txt, name


def test_exported_by_the_library():
    out = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (cm_[a-z0-9_]+)", out))
    assert set(PROTOS) <= exported, sorted(set(PROTOS) - exported)


def test_binding_types_match_the_header():
    from classmate_hip import _lib
    for name in PROTOS:       # every argument is a pointer: the handle, then host arrays / out values
        restype, *args = _lib.SIGNATURES[name]
        n_args = PROTOS[name].count(",") + 1
        assert restype is ctypes.c_int and args == [ctypes.c_void_p] * n_args, name
        assert _lib.fn[name].argtypes == [ctypes.c_void_p] * n_args and _lib.fn[name].restype is ctypes.c_int


def test_null_handle_is_einval_without_a_device():
    import numpy as np
    import pytest
    from classmate_hip import _lib
    mu = np.zeros(768, np.float32)
    sums = np.zeros(768, np.float64)
    n = ctypes.c_int64(-1)
    flag = ctypes.c_int32(-1)
    for rc in (_lib.fn["cm_dense_set_center"](None, _lib.ptr(mu)),
               _lib.fn["cm_dense_set_center"](None, None),
               _lib.fn["cm_dense_get_center"](None, _lib.ptr(mu), ctypes.byref(flag)),
               _lib.fn["cm_dense_mean"](None, _lib.ptr(mu), ctypes.byref(n)),
               _lib.fn["cm_dense_column_sums"](None, _lib.ptr(sums), ctypes.byref(n))):
        assert rc == _lib.CM_EINVAL
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert n.value == -1 and flag.value == -1
