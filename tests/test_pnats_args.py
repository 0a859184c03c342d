"""`rustlight-amd ... point-normal-ats`: the argument errors the CLI reports before it opens a device (no GPU needed), each on one line that names the word,
exit code 2, no file written; the well-formed lines, which get as far as the device, with and without `-x ats` in front; and `point-normal`,
`point-normal-mis` and `point-normal-taylor`, which still refuse `-x ats`."""
import os

from rustlight_amd import api
from tests import cli
from tests.test_pn_args import FLAVOURED

CMD = "point-normal-ats"
WARP_AND_BEST = tuple(n for n in FLAVOURED if n not in api.PN_TAYLOR_STRATEGIES)      # the six warp / best names


def test_the_names_are_the_seven_plain_and_the_six_taylor_names():
    assert len(api.PN_ATS_STRATEGIES) == 13 and len(set(api.PN_ATS_STRATEGIES)) == 13 and len(WARP_AND_BEST) == 6
    assert not set(WARP_AND_BEST) & set(api.PN_ATS_STRATEGIES)


def test_warp_and_best_strategies_are_refused_by_name(built, tmp_path):
    for name in WARP_AND_BEST:
        r = cli.run_cli(tmp_path, CMD, "-s", name)
        assert r.returncode == 2 and name in r.stderr and "not built" in r.stderr and CMD in r.stderr and r.stderr.count("\n") == 1, (name, r.stderr)
        assert not os.path.exists(tmp_path / "out.pfm")


def test_point_normal_ats_argument_errors(built, tmp_path):
    for args, word in (((CMD, "-s", "ats"), "invalid strategy: ats"),
                       ((CMD, "--strategy", "EQ_EX"), "invalid strategy: EQ_EX"),
                       ((CMD, "-s", "pn_taylor_ex"), "invalid strategy: pn_taylor_ex"),
                       ((CMD, "-x"), "point-normal-ats: -x"),
                       ((CMD, "--use-mis"), "point-normal-ats: --use-mis"),
                       ((CMD, "-k", "0.5"), "point-normal-ats: -k"),
                       ((CMD, "--splitting", "0.5"), "point-normal-ats: --splitting"),
                       ((CMD, "-w", "PT"), "point-normal-ats: -w"),
                       ((CMD, "--warps", "N"), "point-normal-ats: --warps"),
                       ((CMD, "--warps-strategy", "B"), "point-normal-ats: --warps-strategy"),
                       ((CMD, "-s", "pn_ex", "-k", "2"), "-k"),
                       (("-x", "ats", CMD, "-k", "2"), "-k"),
                       (("-r", "stratified:3", CMD), "stratified"),
                       (("--numerics", "fast", CMD), "fast"),
                       (("--gpus", "2", CMD), "--gpus"),
                       (("-a", "3", CMD), "-a"),
                       (("-e", "3", CMD), "-e"),
                       (("--frames-in-flight", "2", CMD), "--frames-in-flight"),
                       ((CMD, "--light-streams", "per-path"), "--light-streams"),
                       ((CMD, "--tree-build", "device"), "--tree-build"),
                       ((CMD, "-n", "3"), "point-normal-ats option"),
                       ((CMD, "-m", "3"), "point-normal-ats option"),
                       (("-z", CMD), "unknown option -z")):
        cli.assert_refused(tmp_path, args, word)
    # an invalid strategy lists the thirteen names
    r = cli.run_cli(tmp_path, CMD, "-s", "nope")
    assert all(name in r.stderr for name in api.PN_ATS_STRATEGIES)


def test_point_normal_ats_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        cli.assert_refused(tmp_path, (CMD,), "medium", medium=medium)
        cli.assert_refused(tmp_path, ("-x", "ats", CMD), "medium", medium=medium)


def test_pn_phase_taylor_ex_needs_a_nonzero_g(built, tmp_path):
    for medium in (("-m", "1.0"), ("-m", "1.0:0.2:0")):
        cli.assert_refused(tmp_path, (CMD, "-s", "pn_phase_taylor_ex"), "g != 0", medium=medium)
    cli.assert_reaches_device(tmp_path, (CMD, "-s", "pn_phase_taylor_ex"), medium=("-m", "1.0:0.2:0.6"))


def test_the_other_point_normal_words_still_refuse_the_tree(built, tmp_path):
    for cmd in ("point-normal", "point-normal-mis", "point-normal-taylor"):
        r = cli.assert_refused(tmp_path, ("-x", "ats", cmd), "-x ats is not built")
        assert cmd in r.stderr


def test_point_normal_ats_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the default, every name, both spellings, AA off, both stream modes, `-x ats` in front or not) get as far as opening a device:
    without one, the no-fallback refusal."""
    lines = [(CMD,), ("-x", "ats", CMD), (CMD, "-z"), (CMD, "--disable-aa", "--strategy", "pn_ex"), ("--stream-mode", "per-sample", CMD, "-s", "eq_clamped_ex", "-z"),
             ("--stream-mode", "reference", "-x", "ats", CMD, "-s", "eq_tr_taylor_ex")]
    lines += [(CMD, "-s", s) for s in api.PN_ATS_STRATEGIES if s != "pn_phase_taylor_ex"]
    for args in lines:
        cli.assert_reaches_device(tmp_path, args)
