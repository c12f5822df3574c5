"""bp_gens_direct_tables_check without a GPU: the refusals, the NULL output arrays, the constants of the header and the Python wrapper."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import _lib

    return _lib


@pytest.fixture(params=[0, 1], ids=["secq256k1", "zorro"])
def hostonly(request, L):
    ctx = C.c_void_p()
    assert L.lib().bp_debug_ctx_create_hostonly(request.param, C.c_size_t(16), C.byref(ctx)) == 0
    yield ctx
    L.lib().bp_ctx_destroy(ctx)


def arrays():
    return [(C.c_uint64 * 4)(*([7] * 4)) for _ in range(3)]


def test_null_ctx_is_an_argument_error(L):
    a = arrays()
    assert L.lib().bp_gens_direct_tables_check(None, *a) == L.BP_E_ARG
    assert L.lib().bp_gens_direct_tables_check(None, None, None, None) == L.BP_E_ARG
    assert [list(x) for x in a] == [[7] * 4] * 3          # nothing written


def test_host_only_ctx_has_no_device(L, hostonly):
    a = arrays()
    assert L.lib().bp_gens_direct_tables_check(hostonly, *a) == L.BP_E_NO_DEVICE
    assert [list(x) for x in a] == [[7] * 4] * 3


def test_null_output_arrays_pass_the_argument_checks(L, hostonly):
    """each of the three arrays may be NULL: a host-only ctx gets as far as the device test whichever are given"""
    a = arrays()
    for mask in range(8):
        args = [a[i] if mask >> i & 1 else None for i in range(3)]
        assert L.lib().bp_gens_direct_tables_check(hostonly, *args) == L.BP_E_NO_DEVICE


def test_header_constants():
    hdr = open(os.path.join(ROOT, "include", "arkbp.h")).read()
    consts = dict(re.findall(r"^#define (BP_TABLES_[A-Z_]+) (\d+)", hdr, flags=re.M))
    assert consts == {"BP_TABLES_DIRECT": "0", "BP_TABLES_PC_DIRECT": "1", "BP_TABLES_PC_WIDE": "2", "BP_TABLES_RESIDENT": "3", "BP_TABLES_KINDS": "4"}
    assert re.search(r"^int bp_gens_direct_tables_check\(bp_ctx\* ctx, uint64_t bad\[BP_TABLES_KINDS\], uint64_t first_bad\[BP_TABLES_KINDS\], "
                     r"uint64_t checked\[BP_TABLES_KINDS\]\);$", hdr, flags=re.M)
    # the old check keeps its signature
    assert "int bp_gens_tables_check(bp_ctx* ctx, uint64_t* bad_fold_entries, uint64_t* bad_msm_rows);" in hdr


def test_python_wrapper(L):
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E

    assert "bp_gens_direct_tables_check" in L.EXPORTS
    assert (E.TABLES_DIRECT, E.TABLES_PC_DIRECT, E.TABLES_PC_WIDE, E.TABLES_RESIDENT, E.TABLES_KINDS) == (0, 1, 2, 3, 4)
    assert callable(A.Engine.gens_direct_tables_check)
    eng = A.Engine.host_only(0, 16)
    try:
        with pytest.raises(A.ArkbpError) as err:
            eng.gens_direct_tables_check()
        assert err.value.code == L.BP_E_NO_DEVICE
    finally:
        eng.close()
