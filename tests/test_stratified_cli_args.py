"""`rustlight-amd -r stratified[:SEED]`: the argument errors of the stratified sampler, which the CLI reports before it opens a device (no GPU needed),
and the Python constant of the new rl_stream_mode value."""
import os
import re

from rustlight_amd import api
from tests import cli
from tests.cli import ROOT

PLAIN = dict(medium=(), spp="4")      # these lines: 4 spp and no medium


def test_stratified_argument_errors(built, tmp_path):
    r = cli.run_cli(tmp_path, "-r", "stratified:abc", "path", **PLAIN)
    assert r.returncode == 2 and "seed" in r.stderr and "abc" in r.stderr and r.stderr.count("\n") == 1, r.stderr
    for bad in ("stratified:-1", "stratified:", "stratified:18446744073709551616"):
        r = cli.run_cli(tmp_path, "-r", bad, "ao", **PLAIN)
        assert r.returncode == 2 and "seed" in r.stderr, (bad, r.stderr)
    r = cli.run_cli(tmp_path, "-r", "stratified", "--stream-mode", "per-sample", "path", **PLAIN)
    assert r.returncode == 2 and "--stream-mode" in r.stderr and r.stderr.count("\n") == 1, r.stderr
    r = cli.run_cli(tmp_path, "--stream-mode", "reference", "-r", "stratified:3", "direct", **PLAIN)
    assert r.returncode == 2 and "--stream-mode" in r.stderr, r.stderr
    r = cli.run_cli(tmp_path, "-r", "stratified:7", "--numerics", "fast", "path", **PLAIN)
    assert r.returncode == 2 and "fast" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_unknown_sampler_names_both_samplers(built, tmp_path):
    r = cli.run_cli(tmp_path, "-r", "bogus", "path", **PLAIN)
    assert r.returncode == 2 and "bogus" in r.stderr and "stratified" in r.stderr and "independent" in r.stderr, r.stderr


def test_stream_mode_constant_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rustlight_amd.h")).read()
    enum = re.search(r"typedef enum rl_stream_mode \{([^}]*)\} rl_stream_mode;", header).group(1)
    values = {k: int(v) for k, v in re.findall(r"(RL_STREAM_\w+)\s*=\s*(\d+)", enum)}
    assert values == {"RL_STREAM_REFERENCE_ORDER": 0, "RL_STREAM_PER_SAMPLE": 1, "RL_STREAM_STRATIFIED": 2}
    assert api.STREAM_STRATIFIED == values["RL_STREAM_STRATIFIED"]
    assert (api.STREAM_REFERENCE_ORDER, api.STREAM_PER_SAMPLE) == (0, 1)
