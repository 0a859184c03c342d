"""tests/golden/cli_refusals.json (tests/golden/make_cli_refusals.py): every command line of the corpus is refused by the built CLI with the recorded exit code
and the recorded stderr, byte for byte, and writes no file.  No GPU needed: every line ends before a device is opened."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from tests import cli

GOLDEN = os.path.join(cli.ROOT, "tests", "golden", "cli_refusals.json")


def _mismatch(numbered, tmp_path):
    """None where the line gives what was recorded, in a directory of its own, else what it gave."""
    k, e = numbered
    tmp = str(tmp_path / str(k))
    os.mkdir(tmp)
    argv = [a.replace("{SCENE}", cli.SCENE).replace("{TMP}", tmp) for a in e["args"]]
    r = subprocess.run([cli.EXE, *argv], capture_output=True, cwd=tmp, timeout=60)
    want = e["stderr"].replace("{SCENE}", cli.SCENE).replace("{TMP}", tmp).encode()
    if r.returncode == e["exit"] and r.stderr == want and not os.listdir(tmp):
        return None
    return e["args"], r.returncode, r.stderr, os.listdir(tmp)


def test_every_line_of_the_corpus_is_refused_as_recorded(built, tmp_path):
    entries = json.load(open(GOLDEN))
    assert len(entries) >= 400 and {e["exit"] for e in entries} == {1, 2}
    with ThreadPoolExecutor(max_workers=8) as pool:      # the lines are independent, and a process start is most of a line's time
        wrong = [w for w in pool.map(lambda ne: _mismatch(ne, tmp_path), enumerate(entries)) if w]
    assert not wrong, wrong[:10]
