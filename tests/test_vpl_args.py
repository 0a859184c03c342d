"""`rustlight-amd ... vpl`: the argument errors the CLI reports before it opens a device (no GPU needed) and the parsing of --nb-vpl."""
from tests import cli

PLAIN = dict(medium=(), spp="4")      # these lines: 4 spp and no medium


def test_vpl_argument_errors(built, tmp_path):
    for args, word in ((("vpl", "-n", "16"), "--nb-vpl"),
                       (("vpl", "-l", "bsdf"), "-l"),
                       (("vpl", "-v", "emitter"), "-v"),
                       (("-r", "stratified:3", "vpl"), "stratified"),
                       (("--stream-mode", "per-sample", "vpl"), "per-sample"),
                       (("--numerics", "fast", "vpl"), "fast"),
                       (("--gpus", "2", "vpl"), "--gpus"),
                       (("-a", "3", "vpl"), "-a"),
                       (("--frames-in-flight", "2", "vpl"), "--frames-in-flight"),
                       (("vpl", "--nb-vpl", "0"), "--nb-vpl"),
                       (("vpl", "--nb-vpl", "12x"), "--nb-vpl"),
                       (("vpl", "--nb-vpl", str(1 << 21)), "--nb-vpl"),
                       (("vpl", "-s", "all"), "vpl option")):
        cli.assert_refused(tmp_path, args, word, **PLAIN)


def test_vpl_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed `vpl` lines (-b ignored, --nb-vpl, -l / -v, -m / -r with inf) get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("vpl",), ("vpl", "-b", "0.5", "--nb-vpl", "64", "-l", "volume", "-v", "surface", "-m", "6", "-r", "inf"), ("vpl", "-m", "4", "-r", "2")):
        cli.assert_reaches_device(tmp_path, args, **PLAIN)
