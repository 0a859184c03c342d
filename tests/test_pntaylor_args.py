"""`rustlight-amd ... point-normal-taylor`: the argument errors the CLI reports before it opens a device (no GPU needed), each on one line that names the
word, exit code 2, no file written; the well-formed lines, which get as far as the device; and `point-normal`, which still refuses the six names."""
import os

from rustlight_amd import api
from tests import cli
from tests.test_pn_args import FLAVOURED

CMD = "point-normal-taylor"
NOT_TAYLOR = tuple(n for n in FLAVOURED if n not in api.PN_TAYLOR_STRATEGIES)      # the six warp / best names


def test_the_six_names_are_the_references_taylor_names():
    assert len(api.PN_TAYLOR_STRATEGIES) == 6 and set(api.PN_TAYLOR_STRATEGIES) <= set(FLAVOURED) and len(NOT_TAYLOR) == 6
    assert all("taylor" in n for n in api.PN_TAYLOR_STRATEGIES) and not any("taylor" in n for n in NOT_TAYLOR)


def test_plain_warp_and_best_strategies_are_refused_by_name(built, tmp_path):
    for name in api.PN_STRATEGIES + NOT_TAYLOR:
        r = cli.run_cli(tmp_path, CMD, "-s", name)
        assert r.returncode == 2 and name in r.stderr and "not built" in r.stderr and CMD in r.stderr and r.stderr.count("\n") == 1, (name, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_point_normal_taylor_argument_errors(built, tmp_path):
    for args, word in (((CMD, "-s", "taylor"), "invalid strategy: taylor"),
                       ((CMD, "--strategy", "EQ_TR_TAYLOR_EX"), "invalid strategy: EQ_TR_TAYLOR_EX"),
                       ((CMD, "-s", "pn_taylor_ex"), "invalid strategy: pn_taylor_ex"),
                       ((CMD, "-x"), "point-normal-taylor: -x"),
                       ((CMD, "--use-mis"), "point-normal-taylor: --use-mis"),
                       ((CMD, "-k", "0.5"), "point-normal-taylor: -k"),
                       ((CMD, "--splitting", "0.5"), "point-normal-taylor: --splitting"),
                       ((CMD, "-w", "PT"), "point-normal-taylor: -w"),
                       ((CMD, "--warps", "N"), "point-normal-taylor: --warps"),
                       ((CMD, "--warps-strategy", "B"), "point-normal-taylor: --warps-strategy"),
                       ((CMD, "-s", "pn_tr_taylor_ex", "-k", "2"), "-k"),
                       (("-x", "ats", CMD), "ats"),
                       (("-r", "stratified:3", CMD), "stratified"),
                       (("--numerics", "fast", CMD), "fast"),
                       (("--gpus", "2", CMD), "--gpus"),
                       (("-a", "3", CMD), "-a"),
                       (("-e", "3", CMD), "-e"),
                       (("--frames-in-flight", "2", CMD), "--frames-in-flight"),
                       ((CMD, "--light-streams", "per-path"), "--light-streams"),
                       ((CMD, "--tree-build", "device"), "--tree-build"),
                       ((CMD, "-n", "3"), "point-normal-taylor option"),
                       ((CMD, "-m", "3"), "point-normal-taylor option"),
                       (("-z", CMD), "unknown option -z")):
        cli.assert_refused(tmp_path, args, word)
    # an invalid strategy lists the six names
    r = cli.run_cli(tmp_path, CMD, "-s", "nope")
    assert all(name in r.stderr for name in api.PN_TAYLOR_STRATEGIES)


def test_point_normal_taylor_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        cli.assert_refused(tmp_path, (CMD,), "medium", medium=medium)


def test_pn_phase_taylor_ex_needs_a_nonzero_g(built, tmp_path):
    """assert!(g != 0.0) (point_normal.rs:1414): an isotropic medium, or Henyey-Greenstein with g = 0, exits 2 before a device is opened."""
    for medium in (("-m", "1.0"), ("-m", "1.0:0.2"), ("-m", "1.0:0.2:0"), ("-m", "1.0:0.2:0.0")):
        cli.assert_refused(tmp_path, (CMD, "-s", "pn_phase_taylor_ex"), "g != 0", medium=medium)
    cli.assert_reaches_device(tmp_path, (CMD, "-s", "pn_phase_taylor_ex"), medium=("-m", "1.0:0.2:0.6"))
    cli.assert_reaches_device(tmp_path, (CMD, "-s", "pn_phase_taylor_ex"), medium=("-m", "1.0:0:-0.3"))


def test_point_normal_still_refuses_the_six_names(built, tmp_path):
    for cmd in ("point-normal", "point-normal-mis"):
        for name in api.PN_TAYLOR_STRATEGIES:
            r = cli.run_cli(tmp_path, cmd, "-s", name)
            assert r.returncode == 2 and name in r.stderr and "not built" in r.stderr and r.stderr.count("\n") == 1, (cmd, name, r.stderr)


def test_point_normal_taylor_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the default, every name, both spellings, AA off, both stream modes) get as far as opening a device: without one, the no-fallback
    refusal."""
    lines = [(CMD,), (CMD, "-z"), (CMD, "--disable-aa", "--strategy", "pn_tr_taylor_ex"), ("--stream-mode", "per-sample", CMD, "-s", "eq_clamped_tr_taylor_ex", "-z"),
             ("--stream-mode", "reference", CMD, "-s", "eq_tr_taylor_ex")]
    lines += [(CMD, "-s", s) for s in api.PN_TAYLOR_STRATEGIES if s != "pn_phase_taylor_ex"]
    for args in lines:
        cli.assert_reaches_device(tmp_path, args)
