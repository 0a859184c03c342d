"""`rustlight-amd ... plane-single`: the argument errors the CLI reports before it opens a device (no GPU needed) and the lines that parse."""
from rustlight_amd import api
from tests import cli


def test_plane_single_argument_errors(built, tmp_path):
    for args, word in ((("plane-single", "-s", "valpha"), "valpha is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)"),
                       (("plane-single", "--strategy", "AVERAGE"), "not a correct strategy choice"),
                       (("-r", "stratified:3", "plane-single"), "stratified"),
                       (("--stream-mode", "per-sample", "plane-single"), "per-sample"),
                       (("--numerics", "fast", "plane-single"), "fast"),
                       (("--gpus", "2", "plane-single"), "--gpus"),
                       (("-a", "3", "plane-single"), "-a"),
                       (("-e", "3", "plane-single"), "-e"),
                       (("--frames-in-flight", "2", "plane-single"), "--frames-in-flight"),
                       (("plane-single", "-n", "0"), "--nb-primitive"),
                       (("plane-single", "--nb-primitive", "12x"), "--nb-primitive"),
                       (("plane-single", "-n", str((1 << 20) + 1)), "--nb-primitive"),
                       (("plane-single", "--light-streams", "per-path"), "vpl and vol-primitivies only"),
                       (("plane-single", "--tree-build", "device"), "vol-primitivies only"),
                       (("plane-single", "-m", "3"), "plane-single option"),
                       (("plane-single", "-p", "plane"), "plane-single option")):
        cli.assert_refused(tmp_path, args, word)


def test_plane_single_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        cli.assert_refused(tmp_path, ("plane-single",), "medium", medium=medium)


def test_unknown_subcommand_lists_plane_single(built, tmp_path):
    r = cli.run_cli(tmp_path, "uncorrelated-plane-single")
    assert r.returncode == 2 and "`plane-single`" in r.stderr and r.stderr.count("\n") == 1, r.stderr


def test_plane_single_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the defaults, every strategy, both spellings of the options) get as far as opening a device: without one, the no-fallback refusal."""
    lines = [("plane-single",), ("plane-single", "--nb-primitive", "16", "--strategy", "cmis")]
    lines += [("plane-single", "-n", "8", "-s", s) for s in api.PLANE_STRATEGIES]
    for args in lines:
        cli.assert_reaches_device(tmp_path, args)
