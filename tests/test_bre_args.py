"""`rustlight-amd ... vol-primitivies`: the argument errors the CLI reports before it opens a device (no GPU needed), the primitives that are not built,
and the lines that parse."""
from tests import cli


def test_vol_primitives_argument_errors(built, tmp_path):
    for args, word in ((("vol-primitivies", "-p", "beam"), "not built"),
                       (("vol-primitivies", "-p", "plane"), "not built"),
                       (("vol-primitives", "-p", "vrl"), "not built"),
                       (("vol-primitivies", "-p", "BRE"), "not a correct primitive"),      # the reference's own default string: it matches none of its arms
                       (("-r", "stratified:3", "vol-primitivies"), "stratified"),
                       (("--stream-mode", "per-sample", "vol-primitivies"), "per-sample"),
                       (("--numerics", "fast", "vol-primitivies"), "fast"),
                       (("--gpus", "2", "vol-primitivies"), "--gpus"),
                       (("-a", "3", "vol-primitivies"), "-a"),
                       (("--frames-in-flight", "2", "vol-primitivies"), "--frames-in-flight"),
                       (("vol-primitivies", "--nb-primitive", "0"), "--nb-primitive"),
                       (("vol-primitivies", "--nb-primitive", "12x"), "--nb-primitive"),
                       (("vol-primitivies", "--nb-primitive", str(1 << 21)), "--nb-primitive"),
                       (("vol-primitivies", "--radius", "0"), "--radius"),
                       (("vol-primitivies", "--radius", "-0.1"), "--radius"),
                       (("vol-primitivies", "--radius", "nan"), "--radius"),
                       (("vol-primitivies", "--radius", "inf"), "--radius"),
                       (("vol-primitivies", "--radius", "0.1x"), "--radius"),
                       (("vol-primitivies", "-s", "all"), "vol-primitivies option")):
        cli.assert_refused(tmp_path, args, word)


def test_vol_primitives_options_parse_up_to_the_device(built, tmp_path):
    """Well-formed lines (-p defaults to bre, -n parsed and ignored, the alias) get as far as opening a device: without one, the no-fallback refusal."""
    for args in (("vol-primitivies",), ("vol-primitives", "-p", "bre", "--nb-primitive", "64", "--radius", "0.2", "-n", "3", "-m", "6", "-r", "inf")):
        cli.assert_reaches_device(tmp_path, args)
