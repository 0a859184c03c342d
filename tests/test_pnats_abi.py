"""rl_point_normal_ats_params in its three copies — include/rustlight_amd.h, the ctypes mirror api.PointNormalAtsParams and the #[repr(C)] block of
INTEGRATION.md — held field by field as tests/test_pntaylor_abi.py holds rl_point_normal_taylor_params: rl_point_normal_params' fields and then the family,
declared in two statements (so that the list of tests/test_abi_layout.py stays as it is); rl_pn_ats_family's two values; the symbols in every layer; the units
and launchers; the defaults; and that nothing of the existing header moved."""
import ctypes as C
import os
import re
import subprocess

from rustlight_amd import api
from tests.test_abi_layout import HEADER, _rust_layout, _strip_comments, rust_structs

NAME = "rl_point_normal_ats_params"


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


def test_point_normal_ats_params_layout_in_all_three_copies(tmp_path):
    fields = _header_fields()
    assert fields == ["spp", "strategy", "use_aa", "stream_mode", "seed_variant", "shard_index", "shard_count", "family"]
    src = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {", f'    printf("S %zu\\n", sizeof({NAME}));']
    src += [f'    printf("F {f} %zu %zu\\n", offsetof({NAME}, {f}), sizeof((({NAME}*)0)->{f}));' for f in fields]
    src += ["    return 0;", "}"]
    c_file, exe = tmp_path / "pnats_layout.c", tmp_path / "pnats_layout"
    c_file.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(c_file), "-o", str(exe)])
    size, truth = None, []
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        p = line.split()
        if p[0] == "S":
            size = int(p[1])
        else:
            truth.append((p[1], int(p[2]), int(p[3])))
    cls = api.PointNormalAtsParams
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


def test_point_normal_ats_is_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(HEADER))
    hdr = open(HEADER).read()
    rust = open(os.path.join(root, "INTEGRATION.md")).read()
    hpp = open(os.path.join(root, "rustlight_amd", "csrc", "host", "integrator.hpp")).read()
    for sym in ("rl_point_normal_ats_params_default", "rl_render_point_normal_ats"):
        assert sym in api.PUBLIC_SYMBOLS and re.search(r"\b" + sym + r"\s*\(", hdr) and "pub fn " + sym in rust and sym in hpp
    assert "struct IntegratorPointNormalAts" in hpp and hasattr(api, "IntegratorPointNormalAts") and hasattr(api.Context, "render_point_normal_ats")
    # rl_point_normal_params' fields, then the family, in every copy
    assert api.PointNormalAtsParams._fields_ == api.PointNormalParams._fields_ + [("family", C.c_int32)]
    assert rust_structs()[NAME][:-1] == rust_structs()["rl_point_normal_params"] and rust_structs()[NAME][-1][0] == "family"
    # the units are in the build's list and the launchers in launch.h
    from rustlight_amd import build
    assert {"kernels/pnats_lds.hip", "kernels/pnats_stream.hip"} <= set(build.HIP_SOURCES)
    launch = open(os.path.join(root, "rustlight_amd", "csrc", "kernels", "launch.h")).read()
    assert "launch_pnats_lds(" in launch and "launch_pnats_stream(" in launch
    # rl_pn_ats_family: plain, Taylor
    enum = re.search(r"typedef enum rl_pn_ats_family \{(.*?)\}", _strip_comments(hdr), flags=re.S).group(1)
    assert [(n.strip(), int(v)) for n, v in (item.split("=") for item in enum.split(","))] == [("RL_PN_ATS_PLAIN", 0), ("RL_PN_ATS_TAYLOR", 1)]
    # the names: the seven plain ones, then the six Taylor ones, each with its family's value
    assert api.PN_ATS_STRATEGIES == api.PN_STRATEGIES + api.PN_TAYLOR_STRATEGIES
    assert [api.pn_ats_strategy(n) for n in api.PN_ATS_STRATEGIES] == [(0, i) for i in range(7)] + [(1, i) for i in range(6)]


def test_the_existing_structs_kept_their_text():
    """Nothing of the existing header changes: the three earlier point-normal structs and their enums stand as they stood."""
    text = _strip_comments(open(HEADER).read())
    for name in ("rl_point_normal_params", "rl_point_normal_mis_params", "rl_point_normal_taylor_params"):
        m = re.search(r"struct\s+" + name + r"\s*\{(.*?)\}\s*;", text, flags=re.S)
        assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == ["spp", "strategy", "use_aa", "stream_mode", "seed_variant", "shard_index", "shard_count"], name
    assert re.search(r"typedef enum rl_pn_strategy \{[^}]*RL_PN_PN_EX = 6 \}", text) and re.search(r"typedef enum rl_pn_taylor_strategy \{[^}]*RL_PN_TAYLOR_PN_PHASE = 5 \}", text)


def test_point_normal_ats_params_defaults(built):
    p = api.PointNormalAtsParams()
    api.lib().rl_point_normal_ats_params_default(C.byref(p))
    assert (p.spp, p.family, api.PN_STRATEGIES[p.strategy], p.use_aa, p.stream_mode, p.seed_variant, p.shard_index, p.shard_count) == \
        (1, 0, "eq_ex", 1, api.STREAM_REFERENCE_ORDER, 0, 0, 1)


def test_the_library_exports_the_entry_points(built):
    L = api.lib()
    assert all(hasattr(L, sym) for sym in ("rl_point_normal_ats_params_default", "rl_render_point_normal_ats"))
