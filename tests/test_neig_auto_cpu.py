"""bigKRLS(Neig="auto") without a GPU: the new exports, the untouched options struct and the refusals that come before
any native call."""
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


def test_fit_options_stay_what_they_were(tmp_path):
    """The rank search has an entry point of its own (bigkrls_fit_auto, the cap as an argument): the options struct of
    bigkrls_fit keeps its size and fields, in Python as in the header, so callers built against it are served as
    before."""
    from bigkrls_amd import _lib
    names = [f[0] for f in _lib.FitOptions._fields_]
    assert names[-1] == "n_which" and len(names) == 13 and C.sizeof(_lib.FitOptions) == 88
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "bigkrls.h"\n'
                   'int main(void){printf("%zu %zu\\n", sizeof(bigkrls_fit_options), sizeof(bigkrls_fit_outputs));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.FitOptions), C.sizeof(_lib.FitOutputs)]


def test_fit_auto_is_declared_and_bound():
    from bigkrls_amd import _lib
    m = re.search(r"int\s+bigkrls_fit_auto\s*\(([^;]*)\)\s*;", _header())
    assert m, "bigkrls_fit_auto is not declared in include/bigkrls.h"
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert len(_lib.SIGNATURES["bigkrls_fit_auto"]) == len(args) == len(_lib.SIGNATURES["bigkrls_fit"]) + 1
    assert args[6] == "int64_t neig_max"                                          # between the options and the outputs


def test_eigen_auto_is_declared_and_bound():
    from bigkrls_amd import _lib, ops
    m = re.search(r"int\s+bigkrls_dev_eigen_auto\s*\(([^;]*)\)\s*;", _header())
    assert m, "bigkrls_dev_eigen_auto is not declared in include/bigkrls.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert len(_lib.SIGNATURES["bigkrls_dev_eigen_auto"]) == nargs == 15
    assert callable(ops.bEigenAuto)


class NoContext:                                                                  # (a Context would initialise the GPU)
    handle = None


@pytest.mark.parametrize("n,kwargs,needle", [
    (1200, dict(comm=True), "comm"),
    (1200, dict(), "pass eigtrunc"),                                              # eigtrunc 0 by the n <= 3000 default
    (4000, dict(eigtrunc=0.0), "pass eigtrunc"),                                  # ... and given
    (3200, dict(eigtrunc=0), "pass eigtrunc"),
    (1000, dict(eigtrunc=0.01), "N >= 1024"),
    (1200, dict(eigtrunc=0.01, Neig="all"), '"auto"'),
])
@pytest.mark.parametrize("kernel", ["stored", "implicit"])
def test_auto_arguments_are_refused_before_any_native_call(monkeypatch, kernel, n, kwargs, needle):
    from bigkrls_amd import _lib, api

    def reached(*a, **k):
        raise AssertionError("native code reached")
    monkeypatch.setattr(_lib, "call", reached)
    kwargs = dict(kwargs)
    comm = type("Comm", (), {"ctx": NoContext(), "handle": None})() if kwargs.pop("comm", None) else None
    kwargs.setdefault("Neig", "auto")
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((n, 3)), rng.standard_normal(n)
    with pytest.raises(ValueError) as e:
        api.bigKRLS(y, X, kernel=kernel, vcov_form="factors", ctx=NoContext(), comm=comm, **kwargs)
    assert needle in str(e.value)


def test_the_cap_error_names_the_fix(monkeypatch):
    """The library's cap error (BIGKRLS_EINVAL of the eigensolver) becomes a ValueError that says what to change."""
    from bigkrls_amd import _lib, api

    def native(name, *a):
        raise _lib.BigKRLSError(_lib.EINVAL, "eigen (Krylov, auto rank): more than kcap = 100 eigenvalues reach the "
                                "threshold: theta_kcap / theta_1 = 4.0e-03 is still above keep_thresh = 1.0e-03")
    monkeypatch.setattr(_lib, "call", native)

    class Ctx(NoContext):
        def empty(self, *shape):
            return type("M", (), {"ptr": None})()
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((4000, 3)), rng.standard_normal(4000)
    with pytest.raises(ValueError, match="raise max_factors.*or pass Neig"):
        api.bigKRLS(y, X, Neig="auto", kernel="implicit", vcov_form="factors", max_factors=100, ctx=Ctx())
