"""cm_bm25_filter_eps_multi and cm_bm25_last_eps_passes, the parts that need no GPU: the symbols in
the header and the binding table, and the argument checks that run before any device call."""
import ctypes
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]


def test_symbols_in_header_and_binding_table():
    from classmate_hip import _lib
    header = (REPO / "include" / "classmate_hip.h").read_text()
    for name in ("cm_bm25_filter_eps_multi", "cm_bm25_last_eps_passes"):
        assert f"{name}(cm_bm25 *h" in header
        assert name in _lib.SIGNATURES and callable(_lib.fn[name])
    assert len(_lib.SIGNATURES["cm_bm25_filter_eps_multi"]) == 5       # the return type and four arguments
    assert len(_lib.SIGNATURES["cm_bm25_last_eps_passes"]) == 2


def _call(h, n_filters=1, null=None):
    from classmate_hip import _lib
    a = dict(allow=np.zeros(max(n_filters, 1), np.uint32), eps=np.full(max(n_filters, 1), 7.0))
    p = {name: None if name == null else _lib.ptr(v) for name, v in a.items()}
    return _lib.fn["cm_bm25_filter_eps_multi"](h, p["allow"], n_filters, p["eps"]), a["eps"]


def test_argument_checks_run_before_any_device_call():
    from classmate_hip import _lib
    assert _call(None)[0] == _lib.CM_EINVAL and "NULL" in _lib.last_error()
    assert _lib.fn["cm_bm25_last_eps_passes"](None) == -1
    # the remaining checks read only the arguments: a handle that is never dereferenced
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(4096)))
    for name in ("allow", "eps"):
        assert _call(fake, null=name)[0] == _lib.CM_EINVAL, name
        assert "NULL" in _lib.last_error()
    for n in (-1, -(2 ** 31)):
        assert _call(fake, n_filters=n)[0] == _lib.CM_EINVAL
        assert "n_filters" in _lib.last_error()
    rc, eps = _call(fake, n_filters=0)
    assert rc == _lib.CM_OK and (eps == 7.0).all()                     # nothing done
