"""`rustlight-amd ... plane-single --uncorrelated`: the argument errors the CLI reports before it opens a device (no GPU needed) and the lines that parse."""
from rustlight_amd import api
from tests import cli

CMD = ("plane-single", "--uncorrelated")


def test_uncorrelated_argument_errors(built, tmp_path):
    """What plane-single refuses, with its error text, wherever --uncorrelated stands among the subcommand's options."""
    for args, word in (((*CMD, "-s", "valpha"), "valpha is not a correct strategy choice (uv, ut, vt, average, discrete_mis, valpha, cmis)"),
                       (("plane-single", "--strategy", "AVERAGE", "--uncorrelated"), "not a correct strategy choice"),
                       (("-r", "stratified:3", *CMD), "stratified"),
                       (("--stream-mode", "per-sample", *CMD), "per-sample"),
                       (("--numerics", "fast", *CMD), "fast"),
                       (("--gpus", "2", *CMD), "--gpus"),
                       (("-a", "3", *CMD), "-a"),
                       (("-e", "3", *CMD), "-e"),
                       (("--frames-in-flight", "2", *CMD), "--frames-in-flight"),
                       ((*CMD, "-n", "0"), "--nb-primitive"),
                       (("plane-single", "--nb-primitive", "12x", "--uncorrelated"), "--nb-primitive"),
                       ((*CMD, "-n", str((1 << 20) + 1)), "--nb-primitive"),
                       ((*CMD, "--light-streams", "per-path"), "vpl and vol-primitivies only"),
                       ((*CMD, "--tree-build", "device"), "vol-primitivies only"),
                       ((*CMD, "-m", "3"), "plane-single option"),
                       ((*CMD, "--uncorrelated=1"), "plane-single option"),
                       (("--uncorrelated", "plane-single"), "unknown option --uncorrelated"),
                       (("path", "--uncorrelated"), "unknown path option --uncorrelated")):
        cli.assert_refused(tmp_path, args, word)


def test_uncorrelated_needs_a_medium(built, tmp_path):
    for medium in ((), ("-m", "0.0"), ("-m", "0:0")):
        cli.assert_refused(tmp_path, CMD, "medium", medium=medium)


def test_uncorrelated_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (the defaults, every strategy, both spellings of the options, the flag before and after them) get as far as opening a device: without
    one, the no-fallback refusal."""
    lines = [CMD, (*CMD, "--nb-primitive", "16", "--strategy", "cmis"), ("plane-single", "-n", "4", "--uncorrelated", "-s", "ut")]
    lines += [(*CMD, "-n", "8", "-s", s) for s in api.PLANE_STRATEGIES]
    for args in lines:
        cli.assert_reaches_device(tmp_path, args)
