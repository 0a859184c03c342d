"""`rustlight-amd ... point-normal-mis`: the argument errors the CLI reports before it opens a device (no GPU needed), each on one line that names the word,
exit code 2, no file written; and the well-formed lines, which get as far as the device."""
import os

from rustlight_amd import api
from tests import cli
from tests.test_pn_args import FLAVOURED

CMD = "point-normal-mis"


def test_flavoured_strategies_are_not_built(built, tmp_path):
    for name in FLAVOURED:
        r = cli.run_cli(tmp_path, CMD, "-s", name)
        assert r.returncode == 2 and name in r.stderr and "not built" in r.stderr and CMD in r.stderr and r.stderr.count("\n") == 1, (name, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_point_normal_mis_argument_errors(built, tmp_path):
    for args, word in (((CMD, "-s", "tr"), "invalid strategy: tr"),
                       ((CMD, "--strategy", "TR_EX"), "invalid strategy: TR_EX"),
                       ((CMD, "-s", "pn_phase"), "invalid strategy: pn_phase"),
                       ((CMD, "-x"), "point-normal-mis: -x"),
                       ((CMD, "--use-mis"), "point-normal-mis: --use-mis"),
                       ((CMD, "-k", "0.5"), "point-normal-mis: -k"),
                       ((CMD, "--splitting", "0.5"), "point-normal-mis: --splitting"),
                       ((CMD, "-w", "PT"), "point-normal-mis: -w"),
                       ((CMD, "--warps", "N"), "point-normal-mis: --warps"),
                       ((CMD, "--warps-strategy", "B"), "point-normal-mis: --warps-strategy"),
                       ((CMD, "-s", "pn_ex", "-k", "2"), "-k"),
                       (("-x", "ats", CMD), "ats"),
                       (("-r", "stratified:3", CMD), "stratified"),
                       (("--numerics", "fast", CMD), "fast"),
                       (("--gpus", "2", CMD), "--gpus"),
                       (("-a", "3", CMD), "-a"),
                       (("-e", "3", CMD), "-e"),
                       (("--frames-in-flight", "2", CMD), "--frames-in-flight"),
                       ((CMD, "--light-streams", "per-path"), "--light-streams"),
                       ((CMD, "--tree-build", "device"), "--tree-build"),
                       ((CMD, "-n", "3"), "point-normal-mis option"),
                       ((CMD, "-m", "3"), "point-normal-mis option"),
                       (("-z", CMD), "unknown option -z")):
        cli.assert_refused(tmp_path, args, word)
    # an invalid strategy lists the seven names
    r = cli.run_cli(tmp_path, CMD, "-s", "nope")
    assert all(name in r.stderr for name in api.PN_STRATEGIES)


def test_point_normal_mis_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        cli.assert_refused(tmp_path, (CMD,), "medium", medium=medium)


def test_unknown_subcommand_lists_point_normal_mis(built, tmp_path):
    r = cli.run_cli(tmp_path, "point_normal_mis")
    assert r.returncode == 2 and "`point-normal-mis`" in r.stderr and "`point-normal`" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_point_normal_mis_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the defaults, every name, both spellings, AA off, both stream modes) get as far as opening a device: without one, the no-fallback
    refusal."""
    lines = [(CMD,), (CMD, "-z"), (CMD, "--disable-aa", "--strategy", "pn_ex"), ("--stream-mode", "per-sample", CMD, "-s", "eq_clamped_phase", "-z"),
             ("--stream-mode", "reference", CMD, "-s", "eq_phase")]
    lines += [(CMD, "-s", s) for s in api.PN_STRATEGIES]
    for args in lines:
        cli.assert_reaches_device(tmp_path, args)
