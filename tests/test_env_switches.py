"""The package reads exactly these EA_* environment variables.  A/B switches whose verdict is in are not
kept as environment reads: a new one has to be added here on purpose."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEPT = {
    "EA_DDP_FORCE",
    "EA_DDP_COLLECTIVE",
    "EA_DEBUG_SYNC",
    "EA_SIDE_STREAM_PROBE",
    "EA_SIDE_STREAM_DEBUG",
    "EA_LOGITS_F32",
    "EA_JOINT_LOGITS_F32",
}

_READS = (
    re.compile(r"""getenv\(\s*["'](EA_\w+)["']"""),
    re.compile(r"""os\.environ[^\n"']*["'](EA_\w+)["']"""),
)


def _sources():
    files = glob.glob(os.path.join(ROOT, "espresso_amd", "**", "*.py"), recursive=True)
    files += glob.glob(os.path.join(ROOT, "espresso_amd", "csrc", "*"))
    files += glob.glob(os.path.join(ROOT, "include", "*"))
    return [f for f in files if os.path.isfile(f) and os.path.splitext(f)[1] in (".py", ".hip", ".h", ".hpp", ".cpp", "")]


def test_only_the_kept_environment_switches_are_read():
    found = {}
    for path in _sources():
        with open(path, errors="replace") as f:
            text = f.read()
        for rx in _READS:
            for name in rx.findall(text):
                found.setdefault(name, set()).add(os.path.relpath(path, ROOT))
    extra = {k: sorted(v) for k, v in found.items() if k not in KEPT}
    assert not extra, "environment switches outside the kept list: {}".format(extra)
    assert set(found) == KEPT, "kept switches no longer read anywhere: {}".format(sorted(KEPT - set(found)))
