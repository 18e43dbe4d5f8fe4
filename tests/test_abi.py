"""The C-ABI library loads and exports every symbol include/mjhip.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

from mujoco_torch_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return native.load_library()


def test_header_entry_points_exported(lib):
    text = open(os.path.join(ROOT, "include", "mjhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(mjh_\w+)\s*\(", text))
    assert {"mjh_model_create", "mjh_model_destroy", "mjh_forward", "mjh_step", "mjh_last_error"} <= names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mjhip.h but not exported"


def test_field_lists_match_header(lib):
    native.check_abi(lib)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mjhip.h")).read()
    assert lib.mjh_abi_version() == int(re.search(r"#define MJH_ABI_VERSION (\d+)", header).group(1))


def test_struct_sizes_match_binding(lib):
    n_data = len(native.LISTS["MJH_DATA_REALS"]) + len(native.LISTS["MJH_DATA_I32"]) + len(native.LISTS["MJH_DATA_I64"]) + len(native.LISTS["MJH_DATA_EXTRA_IN"])
    assert ctypes.sizeof(native.DataPtrs) == 8 * n_data == lib.mjh_sizeof_data()


def test_oracle_exports():
    import pyoracle

    lib = pyoracle.lib()
    for n in ("mjo_step", "mjo_forward", "mjo_max_threads"):
        assert hasattr(lib, n)


_C_KINDS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
_STRUCTS = dict({"mjh" + s.__name__: s for s in native.ARGS.values()}, mjhRayCands=native.RayCands, mjhRenderScene=native.RenderScene,
                mjhRenderParams=native.RenderParams)


def header_fields(text, struct):
    """[(field name, ctypes kind)] of ``typedef struct <struct> { ... }`` in the header text: any pointer is a ``c_void_p``, ``T x[N]`` is ``T * N``."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = re.sub(r"\bconst\b", " ", decl).strip()
        if not decl:
            continue
        base, rest = re.fullmatch(r"(\w+)\s*(.*)", decl, re.S).groups()  # (a `*` binds to its declarator: `void *a, *b`, `int32_t* a`)
        for d in rest.split(","):
            name, n = re.fullmatch(r"[\s*]*(\w+)\s*(?:\[(\d+)\])?", d.strip()).groups()
            kind = ctypes.c_void_p if "*" in d else _C_KINDS[base]
            fields.append((name, kind * int(n) if n else kind))
    return fields


@pytest.mark.parametrize("struct", sorted(_STRUCTS))
def test_args_structs_match_header(struct):
    """The hand-written ctypes field lists of native.py against the struct bodies of include/mjhip.h: the same names, in the same order, of the matching kind
    (int32_t -> c_int32, int64_t -> c_int64, double -> c_double, any pointer -> c_void_p).  No library needed."""
    text = open(os.path.join(ROOT, "include", "mjhip.h")).read()
    want = header_fields(text, struct)
    assert len(want) >= 4
    assert list(_STRUCTS[struct]._fields_) == want


def test_args_table_names_the_six_entry_points():
    assert sorted(native.ARGS) == ["mjh_contact_sensors", "mjh_energy", "mjh_integrate", "mjh_jacobian", "mjh_postconstraint", "mjh_support"]
    text = open(os.path.join(ROOT, "include", "mjhip.h")).read()
    for symbol, struct in native.ARGS.items():  # (each symbol takes the struct the table gives it)
        assert re.search(r"int %s\(const mjhModel\* m, const mjh%s\* args, void\* hip_stream\);" % (symbol, struct.__name__), text), symbol
