"""A diagnostic or A/B build of the library: csrc/build.sh (the only place that names the translation units) with extra compiler
flags into a library of its own.  The compiler's messages are shown, never thrown away."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(flags, out, replace=None):
    """`flags`: e.g. "-DAQG_STAMP"; `out`: the library to write; `replace`: {"unit": "/abs/path/of/another/version.hip"}."""
    env = dict(os.environ, AQG_EXTRA_FLAGS=flags, OUT=out)
    env.pop("OBJDIR", None)                       # build.sh then makes (and removes) an object directory of this build's own
    if replace:
        env["AQG_REPLACE"] = " ".join(f"{unit}={os.path.abspath(path)}" for unit, path in replace.items())
    subprocess.check_call(["bash", os.path.join(ROOT, "alphaquoridorgnn_amd", "csrc", "build.sh")], env=env, stdout=subprocess.DEVNULL)
    return out
