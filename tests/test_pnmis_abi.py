"""rl_point_normal_mis_params in its three copies — include/rustlight_amd.h, the ctypes mirror api.PointNormalMisParams and the #[repr(C)] block of
INTEGRATION.md — held field by field as tests/test_pn_abi.py holds rl_point_normal_params, whose fields it has (declared in two statements like it, so that
the list of tests/test_abi_layout.py stays as it is); the symbols in every layer; the defaults."""
import ctypes as C
import os
import re
import subprocess

from rustlight_amd import api
from tests.test_abi_layout import HEADER, _rust_layout, _strip_comments, rust_structs

NAME = "rl_point_normal_mis_params"


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


def test_point_normal_mis_params_layout_in_all_three_copies(tmp_path):
    fields = _header_fields()
    assert fields == ["spp", "strategy", "use_aa", "stream_mode", "seed_variant", "shard_index", "shard_count"]
    src = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {", f'    printf("S %zu\\n", sizeof({NAME}));']
    src += [f'    printf("F {f} %zu %zu\\n", offsetof({NAME}, {f}), sizeof((({NAME}*)0)->{f}));' for f in fields]
    src += ["    return 0;", "}"]
    c_file, exe = tmp_path / "pnmis_layout.c", tmp_path / "pnmis_layout"
    c_file.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(c_file), "-o", str(exe)])
    size, truth = None, []
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        p = line.split()
        if p[0] == "S":
            size = int(p[1])
        else:
            truth.append((p[1], int(p[2]), int(p[3])))
    cls = api.PointNormalMisParams
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


def test_point_normal_mis_is_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(HEADER))
    hdr = open(HEADER).read()
    rust = open(os.path.join(root, "INTEGRATION.md")).read()
    hpp = open(os.path.join(root, "rustlight_amd", "csrc", "host", "integrator.hpp")).read()
    for sym in ("rl_point_normal_mis_params_default", "rl_render_point_normal_mis"):
        assert sym in api.PUBLIC_SYMBOLS and re.search(r"\b" + sym + r"\s*\(", hdr) and "pub fn " + sym in rust and sym in hpp
    assert "struct IntegratorPointNormalMis" in hpp and hasattr(api, "IntegratorPointNormalMis") and hasattr(api.Context, "render_point_normal_mis")
    # the same fields as rl_point_normal_params, in every copy
    assert api.PointNormalMisParams._fields_ == api.PointNormalParams._fields_
    assert rust_structs()[NAME] == rust_structs()["rl_point_normal_params"]
    # the units are in the build's list and the launchers in launch.h
    from rustlight_amd import build
    assert {"kernels/pnmis_lds.hip", "kernels/pnmis_stream.hip"} <= set(build.HIP_SOURCES)
    launch = open(os.path.join(root, "rustlight_amd", "csrc", "kernels", "launch.h")).read()
    assert "launch_pnmis_lds(" in launch and "launch_pnmis_stream(" in launch


def test_point_normal_mis_params_defaults(built):
    p = api.PointNormalMisParams()
    api.lib().rl_point_normal_mis_params_default(C.byref(p))
    assert (p.spp, api.PN_STRATEGIES[p.strategy], p.use_aa, p.stream_mode, p.seed_variant, p.shard_index, p.shard_count) == (1, "tr_ex", 1, api.STREAM_REFERENCE_ORDER, 0, 0, 1)


def test_the_library_exports_the_entry_points(built):
    L = api.lib()
    assert all(hasattr(L, sym) for sym in ("rl_point_normal_mis_params_default", "rl_render_point_normal_mis"))
