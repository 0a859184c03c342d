"""`rustlight-amd ... photon-beams`: the argument errors the CLI reports before it opens a device (no GPU needed), the lines that parse, and
`vol-primitivies -p beam`, which stays refused: the photon beams have a subcommand of their own."""
from rustlight_amd import api
from tests import cli


def test_photon_beams_argument_errors(built, tmp_path):
    for args, word in ((("-r", "stratified:3", "photon-beams"), "stratified"),
                       (("--stream-mode", "per-sample", "photon-beams"), "per-sample"),
                       (("--numerics", "fast", "photon-beams"), "fast"),
                       (("--gpus", "2", "photon-beams"), "--gpus"),
                       (("-a", "3", "photon-beams"), "-a"),
                       (("-e", "3", "photon-beams"), "-e"),
                       (("--frames-in-flight", "2", "photon-beams"), "--frames-in-flight"),
                       (("photon-beams", "--nb-primitive", "0"), "--nb-primitive"),
                       (("photon-beams", "--nb-primitive", "12x"), "--nb-primitive"),
                       (("photon-beams", "--nb-primitive", str(api.BEAM_MAX + 1)), "--nb-primitive"),
                       (("photon-beams", "--radius", "0"), "--radius"),
                       (("photon-beams", "--radius", "-0.1"), "--radius"),
                       (("photon-beams", "--radius", "nan"), "--radius"),
                       (("photon-beams", "--radius", "inf"), "--radius"),
                       (("photon-beams", "--radius", "0.1x"), "--radius"),
                       (("photon-beams", "--light-streams", "other"), "--light-streams"),
                       (("photon-beams", "--tree-build", "device"), "--tree-build"),
                       (("photon-beams", "-p", "beam"), "photon-beams option"),
                       (("photon-beams", "-s", "all"), "photon-beams option"),
                       (("--light-streams", "per-path", "photon-beams"), "after the subcommand"),
                       (("vol-primitivies", "-p", "beam"), "not built")):
        cli.assert_refused(tmp_path, args, word)


def test_photon_beams_need_a_medium(built, tmp_path):
    r = cli.run_cli(tmp_path, "photon-beams", medium=())
    assert r.returncode == 2 and "needs a medium" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_unknown_subcommand_lists_photon_beams(built, tmp_path):
    r = cli.run_cli(tmp_path, "photon-beam")
    assert r.returncode == 2 and "`photon-beams`" in r.stderr and "`plane-single`" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_photon_beams_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (-n parsed and ignored, both stream modes) get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("photon-beams",), ("photon-beams", "--nb-primitive", str(api.BEAM_MAX), "--radius", "0.2", "-n", "3", "-m", "6", "-r", "inf"),
                 ("photon-beams", "--nb-primitive", "64", "--light-streams", "per-path"), ("photon-beams", "--light-streams", "reference", "-m", "inf")):
        cli.assert_reaches_device(tmp_path, args)
