"""rl_point_normal_params in its three copies — include/rustlight_amd.h, the ctypes mirror api.PointNormalParams and the #[repr(C)] block of INTEGRATION.md —
held field by field as tests/test_abi_layout.py holds the header's other structs (that file pins the ten it knows, and this struct is declared in two
statements so that its list stays as it is); the defaults are the reference CLI's."""
import ctypes as C
import os
import re
import subprocess

from rustlight_amd import api
from tests.test_abi_layout import HEADER, _rust_layout, _strip_comments, rust_structs

NAME = "rl_point_normal_params"


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


def test_point_normal_params_layout_in_all_three_copies(tmp_path):
    fields = _header_fields()
    assert fields == ["spp", "strategy", "use_aa", "stream_mode", "seed_variant", "shard_index", "shard_count"]
    src = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {", f'    printf("S %zu\\n", sizeof({NAME}));']
    src += [f'    printf("F {f} %zu %zu\\n", offsetof({NAME}, {f}), sizeof((({NAME}*)0)->{f}));' for f in fields]
    src += ["    return 0;", "}"]
    c_file, exe = tmp_path / "pn_layout.c", tmp_path / "pn_layout"
    c_file.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", str(c_file), "-o", str(exe)])
    size, truth = None, []
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        p = line.split()
        if p[0] == "S":
            size = int(p[1])
        else:
            truth.append((p[1], int(p[2]), int(p[3])))
    cls = api.PointNormalParams
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


def test_point_normal_is_declared_in_every_layer():
    hdr = open(HEADER).read()
    rust = open(os.path.join(os.path.dirname(os.path.dirname(HEADER)), "INTEGRATION.md")).read()
    hpp = open(os.path.join(os.path.dirname(os.path.dirname(HEADER)), "rustlight_amd", "csrc", "host", "integrator.hpp")).read()
    for sym in ("rl_point_normal_params_default", "rl_render_point_normal"):
        assert sym in api.PUBLIC_SYMBOLS and re.search(r"\b" + sym + r"\s*\(", hdr) and "pub fn " + sym in rust and sym in hpp
    values = re.search(r"typedef enum rl_pn_strategy \{(.*?)\}", hdr, flags=re.S).group(1)
    names = [n.lower()[len("rl_pn_"):] for n in re.findall(r"(RL_PN_\w+)\s*=", values)]
    assert tuple(names) == api.PN_STRATEGIES and [int(v) for v in re.findall(r"=\s*(\d+)", values)] == list(range(7))
    assert "struct IntegratorPointNormal" in hpp and hasattr(api, "IntegratorPointNormal") and hasattr(api.Context, "render_point_normal")


def test_point_normal_params_defaults_are_the_reference_cli_defaults(built):
    p = api.PointNormalParams()
    api.lib().rl_point_normal_params_default(C.byref(p))
    assert (p.spp, api.PN_STRATEGIES[p.strategy], p.use_aa, p.stream_mode, p.seed_variant, p.shard_index, p.shard_count) == (1, "tr_ex", 1, api.STREAM_REFERENCE_ORDER, 0, 0, 1)
