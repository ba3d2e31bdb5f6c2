"""bigKRLS(kernel="implicit") without a GPU: the option field, the new export and the argument validation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "bigkrls.h")) as f:
        return f.read()


def test_kernel_form_sits_where_reserved_sat():
    """The field that was `reserved`: an int32 right behind `acf`, in front of the pointer `which_derivatives`."""
    from bigkrls_amd import _lib
    names = [f[0] for f in _lib.FitOptions._fields_]
    assert "reserved" not in names
    assert names.index("kernel_form") == names.index("acf") + 1 == names.index("which_derivatives") - 1
    assert _lib.FitOptions.kernel_form.size == 4
    assert _lib.FitOptions.kernel_form.offset == _lib.FitOptions.acf.offset + 4
    # 8 + 5 doubles + neig + three int32 in front of it
    assert _lib.FitOptions.kernel_form.offset == 8 + 5 * 8 + 8 + 3 * 4
    assert C.sizeof(_lib.FitOptions) == 88                                     # unchanged: 68 + 4 + pointer + int64


def test_fit_options_size_and_offset_match_the_header(tmp_path):
    from bigkrls_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bigkrls.h"\n'
                   'int main(void){printf("%zu %zu\\n", sizeof(bigkrls_fit_options), '
                   'offsetof(bigkrls_fit_options, kernel_form));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.FitOptions), _lib.FitOptions.kernel_form.offset]


def test_eigen_implicit_is_declared_and_bound():
    from bigkrls_amd import _lib
    m = re.search(r"int\s+bigkrls_dev_eigen_implicit\s*\(([^;]*)\)\s*;", _header())
    assert m, "bigkrls_dev_eigen_implicit is not declared in include/bigkrls.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "bigkrls_dev_eigen" in v)
    assert "bigkrls_dev_eigen_implicit" in table
    assert len(table["bigkrls_dev_eigen_implicit"]) == nargs == 13


@pytest.mark.parametrize("n,kwargs,needle", [
    (1200, dict(vcov_form="factors"), "Neig"),                                    # no Neig
    (1200, dict(Neig=301, vcov_form="factors"), "4 Neig <= N"),                   # Neig > N / 4
    (600, dict(Neig=96, vcov_form="factors"), "N >= 1024"),                       # N too small for the block Lanczos
    (1200, dict(Neig=96, vcov_form="dense"), 'vcov_form="factors"'),
    (1200, dict(Neig=96), 'vcov_form="factors"'),                                 # (the default form is dense)
    (1200, dict(Neig=96, vcov_form="both"), 'vcov_form="factors"'),
    (1200, dict(Neig=96, vcov_form="factors", comm=object()), "comm"),
])
def test_implicit_arguments_are_refused_before_any_native_call(monkeypatch, n, kwargs, needle):
    import bigkrls_amd as bk
    from bigkrls_amd import _lib, api

    def reached(*a, **k):
        raise AssertionError("native code reached")
    monkeypatch.setattr(_lib, "call", reached)

    class NoContext:                                                              # (a Context would initialise the GPU)
        handle = None
    comm = kwargs.pop("comm", None)
    if comm is not None:
        comm = type("Comm", (), {"ctx": NoContext(), "handle": None})()
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    with pytest.raises(ValueError) as e:
        api.bigKRLS(y, X, kernel="implicit", ctx=NoContext(), comm=comm, **kwargs)
    assert needle in str(e.value)
    assert 'kernel="stored"' in str(e.value) or "vcov_form" in str(e.value)      # the message names the fix


def test_unknown_kernel_form_is_refused(monkeypatch):
    from bigkrls_amd import _lib, api
    monkeypatch.setattr(_lib, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("native code reached")))
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="kernel must be"):
        api.bigKRLS(rng.standard_normal(50), rng.standard_normal((50, 2)), kernel="other", ctx=object())
