"""rl_point_normal_taylor_params in its three copies — include/rustlight_amd.h, the ctypes mirror api.PointNormalTaylorParams and the #[repr(C)] block of
INTEGRATION.md — held field by field as tests/test_pntaylor_abi.py holds rl_point_normal_taylor_params: rl_point_normal_params' fields, declared in two statements
(so that the list of tests/test_abi_layout.py stays as it is); rl_pn_taylor_strategy's six values in the order of api.PN_TAYLOR_STRATEGIES; the symbols in
every layer; the units and launchers; the defaults."""
import ctypes as C
import os
import re
import subprocess

from rustlight_amd import api
from tests.test_abi_layout import HEADER, _rust_layout, _strip_comments, rust_structs

NAME = "rl_point_normal_taylor_params"


def _header_fields():
    text = _strip_comments(open(HEADER).read())
    m = re.search(r"struct\s+" + NAME + r"\s*\{(.*?)\}\s*;\s*typedef\s+struct\s+" + NAME + r"\s+" + NAME + r"\s*;", text, flags=re.S)
    assert m, "the struct and its typedef"
    fields = []
    for decl in m.group(1).split(";"):
        for part in decl.strip().split(","):
            if part.strip():
                fields.append(re.search(r"(\w+)\s*$", part.strip()).group(1))
    return fields


def test_point_normal_taylor_params_layout_in_all_three_copies(tmp_path):
    fields = _header_fields()
    assert fields == ["spp", "strategy", "use_aa", "stream_mode", "seed_variant", "shard_index", "shard_count"]
    src = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {", f'    printf("S %zu\\n", sizeof({NAME}));']
    src += [f'    printf("F {f} %zu %zu\\n", offsetof({NAME}, {f}), sizeof((({NAME}*)0)->{f}));' for f in fields]
    src += ["    return 0;", "}"]
    c_file, exe = tmp_path / "pntaylor_layout.c", tmp_path / "pntaylor_layout"
    c_file.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(c_file), "-o", str(exe)])
    size, truth = None, []
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        p = line.split()
        if p[0] == "S":
            size = int(p[1])
        else:
            truth.append((p[1], int(p[2]), int(p[3])))
    cls = api.PointNormalTaylorParams
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == truth
    structs = rust_structs()
    off, align, got = 0, 1, []
    for n, t in structs[NAME]:
        s, a = _rust_layout(t, structs)
        off = (off + a - 1) // a * a
        got.append((n, off, s))
        off += s
        align = max(align, a)
    assert got == truth and (off + align - 1) // align * align == size


def test_point_normal_taylor_is_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(HEADER))
    hdr = open(HEADER).read()
    rust = open(os.path.join(root, "INTEGRATION.md")).read()
    hpp = open(os.path.join(root, "rustlight_amd", "csrc", "host", "integrator.hpp")).read()
    for sym in ("rl_point_normal_taylor_params_default", "rl_render_point_normal_taylor"):
        assert sym in api.PUBLIC_SYMBOLS and re.search(r"\b" + sym + r"\s*\(", hdr) and "pub fn " + sym in rust and sym in hpp
    assert "struct IntegratorPointNormalTaylor" in hpp and hasattr(api, "IntegratorPointNormalTaylor") and hasattr(api.Context, "render_point_normal_taylor")
    # the same fields as rl_point_normal_params, in every copy
    assert api.PointNormalTaylorParams._fields_ == api.PointNormalParams._fields_
    assert rust_structs()[NAME] == rust_structs()["rl_point_normal_params"]
    # the units are in the build's list and the launchers in launch.h
    from rustlight_amd import build
    assert {"kernels/pntaylor_lds.hip", "kernels/pntaylor_stream.hip"} <= set(build.HIP_SOURCES)
    launch = open(os.path.join(root, "rustlight_amd", "csrc", "kernels", "launch.h")).read()
    assert "launch_pntaylor_lds(" in launch and "launch_pntaylor_stream(" in launch
    # rl_pn_taylor_strategy: six values, in the order of the names
    enum = re.search(r"typedef enum rl_pn_taylor_strategy \{(.*?)\}", _strip_comments(hdr), flags=re.S).group(1)
    values = [(n.strip(), int(v)) for n, v in (item.split("=") for item in enum.split(","))]
    assert values == [("RL_PN_TAYLOR_" + n[:-len("_taylor_ex")].upper(), i) for i, n in enumerate(api.PN_TAYLOR_STRATEGIES)]
    assert api.PN_TAYLOR_STRATEGIES == ("eq_phase_taylor_ex", "eq_tr_taylor_ex", "eq_clamped_phase_taylor_ex", "eq_clamped_tr_taylor_ex", "pn_tr_taylor_ex",
                                        "pn_phase_taylor_ex")
    assert not set(api.PN_TAYLOR_STRATEGIES) & set(api.PN_STRATEGIES)


def test_point_normal_taylor_params_defaults(built):
    p = api.PointNormalTaylorParams()
    api.lib().rl_point_normal_taylor_params_default(C.byref(p))
    assert (p.spp, api.PN_TAYLOR_STRATEGIES[p.strategy], p.use_aa, p.stream_mode, p.seed_variant, p.shard_index, p.shard_count) == (1, "eq_tr_taylor_ex", 1, api.STREAM_REFERENCE_ORDER, 0, 0, 1)


def test_the_library_exports_the_entry_points(built):
    L = api.lib()
    assert all(hasattr(L, sym) for sym in ("rl_point_normal_taylor_params_default", "rl_render_point_normal_taylor"))
