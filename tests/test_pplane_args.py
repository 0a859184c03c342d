"""`rustlight-amd ... photon-planes`: the argument errors the CLI reports before it opens a device (no GPU needed) — one line, exit 2, no output file —, the
lines that parse, and `vol-primitivies -p plane`, which stays refused: the photon planes have a subcommand of their own."""
from rustlight_amd import api
from tests import cli


def test_photon_planes_argument_errors(built, tmp_path):
    for args, word in ((("-r", "stratified:3", "photon-planes"), "stratified"),
                       (("--stream-mode", "per-sample", "photon-planes"), "per-sample"),
                       (("--numerics", "fast", "photon-planes"), "fast"),
                       (("--gpus", "2", "photon-planes"), "--gpus"),
                       (("-a", "3", "photon-planes"), "-a"),
                       (("-e", "3", "photon-planes"), "-e"),
                       (("--frames-in-flight", "2", "photon-planes"), "--frames-in-flight"),
                       (("photon-planes", "--nb-primitive", "0"), "--nb-primitive"),
                       (("photon-planes", "--nb-primitive", "12x"), "--nb-primitive"),
                       (("photon-planes", "--nb-primitive", str(api.BEAM_MAX + 1)), "--nb-primitive"),
                       (("photon-planes", "--radius", "0"), "--radius"),
                       (("photon-planes", "--radius", "-0.1"), "--radius"),
                       (("photon-planes", "--radius", "nan"), "--radius"),
                       (("photon-planes", "--radius", "inf"), "--radius"),
                       (("photon-planes", "--radius", "0.1x"), "--radius"),
                       (("photon-planes", "--light-streams", "other"), "--light-streams"),
                       (("photon-planes", "--tree-build", "device"), "--tree-build"),
                       (("photon-planes", "-p", "plane"), "photon-planes option"),
                       (("photon-planes", "-m", "3"), "-m 3"),
                       (("photon-planes", "-m", "1"), "-m 1"),
                       (("photon-planes", "-s", "all"), "photon-planes option"),
                       (("--light-streams", "per-path", "photon-planes"), "after the subcommand"),
                       (("vol-primitivies", "-p", "plane"), "not built")):
        cli.assert_refused(tmp_path, args, word)


def test_photon_planes_need_a_medium(built, tmp_path):
    r = cli.run_cli(tmp_path, "photon-planes", medium=())
    assert r.returncode == 2 and "needs a medium" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_unknown_subcommand_lists_photon_planes(built, tmp_path):
    r = cli.run_cli(tmp_path, "photon-plane")
    assert r.returncode == 2 and "`photon-planes`" in r.stderr and "`photon-beams`" in r.stderr and "`plane-single`" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_photon_planes_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (-n parsed and ignored, both stream modes) get as far as opening a device: without one, the no-fallback refusal.
    Known, and older than the CLI's table (profiles/cli_note.md): on a machine with a GPU the second line fails this test.  It parses and opens the device, and
    the library then refuses the plane pass (exit code 1, "more than RL_BEAM_MAX + 2048 surface beams arose before nb_primitive planes were stored")."""
    for args in (("photon-planes",), ("photon-planes", "--nb-primitive", str(api.BEAM_MAX), "--radius", "0.2", "-n", "3", "-m", "4", "-r", "inf"),
                 ("photon-planes", "--nb-primitive", "64", "--light-streams", "per-path"), ("photon-planes", "--light-streams", "reference", "-m", "inf")):
        cli.assert_reaches_device(tmp_path, args)
