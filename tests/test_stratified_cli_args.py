"""`rustlight-amd -r stratified[:SEED]`: the argument errors of the stratified sampler, which the CLI reports before it opens a device (no GPU needed),
and the Python constant of the new rl_stream_mode value."""
import os
import re
import subprocess

from rustlight_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "data", "cbox.pbrt")


def _cli(tmp_path, *args):
    exe = os.path.join(os.path.dirname(api.LIB_PATH), "rustlight-amd")
    return subprocess.run([exe, SCENE, "-n", "4", "-o", str(tmp_path / "out.pfm"), *args], capture_output=True, text=True, timeout=60)


def test_stratified_argument_errors(built, tmp_path):
    r = _cli(tmp_path, "-r", "stratified:abc", "path")
    assert r.returncode == 2 and "seed" in r.stderr and "abc" in r.stderr and r.stderr.count("\n") == 1, r.stderr
    for bad in ("stratified:-1", "stratified:", "stratified:18446744073709551616"):
        r = _cli(tmp_path, "-r", bad, "ao")
        assert r.returncode == 2 and "seed" in r.stderr, (bad, r.stderr)
    r = _cli(tmp_path, "-r", "stratified", "--stream-mode", "per-sample", "path")
    assert r.returncode == 2 and "--stream-mode" in r.stderr and r.stderr.count("\n") == 1, r.stderr
    r = _cli(tmp_path, "--stream-mode", "reference", "-r", "stratified:3", "direct")
    assert r.returncode == 2 and "--stream-mode" in r.stderr, r.stderr
    r = _cli(tmp_path, "-r", "stratified:7", "--numerics", "fast", "path")
    assert r.returncode == 2 and "fast" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_unknown_sampler_names_both_samplers(built, tmp_path):
    r = _cli(tmp_path, "-r", "bogus", "path")
    assert r.returncode == 2 and "bogus" in r.stderr and "stratified" in r.stderr and "independent" in r.stderr, r.stderr


def test_stream_mode_constant_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rustlight_amd.h")).read()
    enum = re.search(r"typedef enum rl_stream_mode \{([^}]*)\} rl_stream_mode;", header).group(1)
    values = {k: int(v) for k, v in re.findall(r"(RL_STREAM_\w+)\s*=\s*(\d+)", enum)}
    assert values == {"RL_STREAM_REFERENCE_ORDER": 0, "RL_STREAM_PER_SAMPLE": 1, "RL_STREAM_STRATIFIED": 2}
    assert api.STREAM_STRATIFIED == values["RL_STREAM_STRATIFIED"]
    assert (api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE) == (0, 1)
