"""Host-side checks (no GPU) of what the batched API's layers must agree on without a compiler telling them: the
ctypes signature table of hpmpc_amd.bindings against the prototypes of include/hpmpc_mi355x.h, and the LDS
constants of csrc/hpmpc_kargs.h against the horizon bound the plan check reports."""
import ctypes as C
import os
import re
import types

from hpmpc_amd import batch, bindings, ocp_batch, soft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpmpc_amd", "csrc")


def _ctype(decl, is_return=False):
    """The ctypes type of one C declarator (type, or type and name); raises on anything it does not know."""
    decl = " ".join(decl.split())
    if "*" in decl:
        return C.c_char_p if is_return and decl.replace(" ", "") == "constchar*" else C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not is_return:
        assert len(words) >= 2, f"parameter without a name: {decl!r}"
        words = words[:-1]
    return {("void",): None, ("int",): C.c_int, ("double",): C.c_double,
            ("long", "long"): C.c_longlong}[tuple(words)]


def header_signatures():
    """{name: (restype, argtypes)} of every hpmpc_mi355x_* prototype of the header, comments stripped."""
    text = open(os.path.join(ROOT, "include", "hpmpc_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    code = re.sub(r"^\s*#.*$", "", code, flags=re.M)
    out = {}
    # a prototype: a statement (the text between ';', '{' and '}') that names such a function before a '('
    for stmt in re.split(r"[;{}]", code):
        m = re.search(r"\b(hpmpc_mi355x_\w+)\s*\(", stmt)
        if not m:
            continue
        name, ret = m.group(1), stmt[:m.start()].strip()
        assert ret, f"no return type in {stmt!r}"
        args = stmt[m.end():].strip()
        assert args.endswith(")") and "(" not in args, f"cannot read the prototype of {name}: {stmt!r}"
        args = args[:-1].strip()
        assert name not in out, name
        params = [] if args == "void" else [_ctype(a) for a in args.split(",")]
        out[name] = (_ctype(ret, is_return=True), params)
    return out


def test_signature_table_is_the_header():
    want = header_signatures()
    assert len(want) >= 40 and "hpmpc_mi355x_pcond_batch" in want and "hpmpc_mi355x_wide_ipm_batch" in want
    assert set(bindings.SIGNATURES) == set(want), set(bindings.SIGNATURES) ^ set(want)
    for name, (restype, argtypes) in want.items():
        assert bindings.SIGNATURES[name][0] is restype, name
        assert list(bindings.SIGNATURES[name][1]) == argtypes, name
    # the parser itself: a pointer return, const char *, long long, an int among pointers
    assert want["hpmpc_mi355x_version"] == (C.c_char_p, [])
    assert want["hpmpc_mi355x_ws_doubles"] == (C.c_longlong, [C.c_void_p])
    assert want["hpmpc_mi355x_plan_destroy"] == (None, [C.c_void_p])
    assert want["hpmpc_mi355x_pcond_offsets"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])
    assert want["hpmpc_mi355x_ipm_batch"][1][13:17] == [C.c_int, C.c_double, C.c_double, C.c_double]


def test_lib_binds_every_function_of_the_built_library():
    if not os.path.exists(bindings.LIBPATH):
        from hpmpc_amd.build import build_hip

        build_hip()
    L = bindings.lib()
    for name, (restype, argtypes) in bindings.SIGNATURES.items():
        fn = getattr(L, name)  # the built library exports every one
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.hpmpc_mi355x_version().startswith(b"hpmpc_mi355x")
    assert L.hpmpc_mi355x_ws_doubles(None) == 0 and L.hpmpc_mi355x_kkt_scratch_doubles(None) == 0
    # the names the solver modules and the tools import are this one loader
    assert batch.lib is bindings.lib and batch.LIBPATH == bindings.LIBPATH
    assert batch.kkt_lib() is L and ocp_batch.ocp_lib() is L and soft._soft_lib() is L


def test_binding_skips_what_a_library_lacks():
    """An older A/B library (HPMPC_MI355X_LIB) has fewer calls: what it has is declared, what it lacks is left."""
    old = types.SimpleNamespace(hpmpc_mi355x_ipm_batch=types.SimpleNamespace(restype=C.c_int, argtypes=None))
    assert bindings.bind(old) is old
    assert old.hpmpc_mi355x_ipm_batch.argtypes == bindings.SIGNATURES["hpmpc_mi355x_ipm_batch"][1]
    assert not hasattr(old, "hpmpc_mi355x_kkt_new_rhs_batch")


def test_lds_constants_give_the_horizon_bound():
    """LDS_FIXED + LDS_PER_STAGE (N + 1) <= 160 KiB is plan_supported's limit; its message names the largest N."""
    kargs = open(os.path.join(CSRC, "hpmpc_kargs.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, kargs).group(1))
    fixed, per_stage = const("LDS_FIXED"), const("LDS_PER_STAGE")
    n_max = (160 * 1024 - fixed) // per_stage - 1
    assert fixed + per_stage * (n_max + 1) <= 160 * 1024 < fixed + per_stage * (n_max + 2)
    assert n_max == 1571
    capi = open(os.path.join(CSRC, "hpmpc_capi.cpp")).read()
    assert "(N <= %d)" % n_max in capi
    assert "LDS_FIXED + (long long)LDS_PER_STAGE * (N + 1) > 160 * 1024" in capi


def test_lds_struct_sizes_are_written_once():
    """The struct sizes behind the two constants appear in one static_assert, not in every launcher."""
    hits = []
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        hits += [name] * text.count("sizeof(StageInfo) + 40")
    assert hits == ["hk_ipm_body.h"], hits
    body = open(os.path.join(CSRC, "hk_ipm_body.h")).read()
    assert "static_assert(LDS_FIXED == sizeof(Scratch) && LDS_PER_STAGE == sizeof(StageInfo) + 40" in body
