"""No NFS_* switch goes unlisted: every name the sources read stands in tests/switch_runs.py SWITCHES with the test that
holds it, "measurement build only" or "no effect on results" and a reason; docs/switches.md lists the same names.  And the
host-side clamps of the integer switches, through the plan queries (they launch nothing, so they run without a GPU, in a
child process each, the switches being read once per process)."""
import ast
import glob
import os
import re
import subprocess
import sys

from tests import switch_runs as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "neural-flow-style_amd")


def names_read():
    """{name: [file, ...]} of getenv("NFS_...") in csrc/*.hip, csrc/*.h and of os.environ reads in the package's *.py"""
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))):
        for name in re.findall(r'getenv\("(NFS_[A-Z0-9_]+)"\)', open(path).read()):
            found.setdefault(name, []).append(os.path.basename(path))
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        for name in re.findall(r'environ(?:\.get\(|\[|\.pop\()\s*"(NFS_[A-Z0-9_]+)"', open(path).read()):
            found.setdefault(name, []).append(os.path.basename(path))
    return found


def test_the_collector_finds_the_reads():
    found = names_read()
    assert len(found) >= 50
    assert "vgg.hip" in found["NFS_WINOGRAD_TILE"] and "winograd.hip" in found["NFS_WINOGRAD_TILE"]
    assert found["NFS_HIST_WIDE"] == ["ops.py"] and "engine.py" in found["NFS_SLAB_PACK"] and "_lib.py" in found["NFS_LIB_PATH"]


def test_every_switch_read_is_listed_and_nothing_else():
    found = names_read()
    missing = sorted(set(found) - set(SR.SWITCHES))
    assert not missing, "read by the sources, not in switch_runs.SWITCHES: %s" % {k: found[k] for k in missing}
    stale = sorted(set(SR.SWITCHES) - set(found))
    assert not stale, "in switch_runs.SWITCHES, read nowhere: %s" % stale


def _defined_tests(module):
    path = os.path.join(ROOT, *module.split(".")) + ".py"
    if not os.path.exists(path):
        return None
    return {n.name for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_record_is_of_a_known_kind_and_names_an_existing_test():
    for name, (kind, what) in SR.SWITCHES.items():
        assert kind in ("test", SR.MEASUREMENT, SR.NO_EFFECT) and what, name
        if kind == "test":
            module, test = what.split("::")
            tests = _defined_tests(module)
            assert tests is not None, "%s: no module %s" % (name, module)
            assert test in tests, "%s: %s has no %s" % (name, module, test)
            assert name in open(os.path.join(ROOT, *module.split(".")) + ".py").read(), "%s is not named in %s" % (name, module)


def test_measurement_switches_are_read_inside_nfs_ablate_only():
    for name, (kind, _) in SR.SWITCHES.items():
        if kind != SR.MEASUREMENT:
            continue
        for path in glob.glob(os.path.join(PKG, "csrc", "*.hip")):
            depth = 0
            for line in open(path):
                s = line.strip()
                if s.startswith("#ifdef NFS_ABLATE"):
                    depth += 1
                elif s.startswith("#if") and depth:
                    depth += 1
                elif s.startswith("#endif") and depth:
                    depth -= 1
                if 'getenv("%s")' % name in line:
                    assert depth > 0, "%s read outside #ifdef NFS_ABLATE in %s" % (name, os.path.basename(path))


def test_the_readable_table_lists_the_same_names():
    text = open(os.path.join(ROOT, "docs", "switches.md")).read()
    listed = set(re.findall(r"^\| `(NFS_[A-Z0-9_]+)`", text, flags=re.M))
    assert listed == set(SR.SWITCHES), (sorted(set(SR.SWITCHES) - listed), sorted(listed - set(SR.SWITCHES)))
    for name, (kind, what) in SR.SWITCHES.items():
        row = next(line for line in text.splitlines() if line.startswith("| `%s`" % name))
        assert (what.split("::")[1] if kind == "test" else kind) in row, name


# ---- the host clamps, through the queries that launch nothing ----------------------------------------------------------------
_QUERY = r"""
import json, sys
sys.path.insert(0, %r)
import neural_flow_style_amd.ops as ops
from neural_flow_style_amd import _lib
B, H, W = 8, 120, 130
out = dict(c3f=ops.conv3x3_plan(B, H, W, 3, 64), c3d=ops.conv3x3_plan(B, H, W, 64, 3),
           narrow=ops.conv3x3_plan(2, 8, 8, 64, 64)["family"], thin=ops.conv3x3_plan(2, 8, 8, 32, 64)["family"],
           gram=[int(_lib.lib().nfs_gram_workspace_floats(*s)) for s in ((1, 32000, 64), (2, 8224, 128), (1, 1000, 128))])
print("RESULT " + json.dumps(out))
""" % ROOT


def _query(env):
    import json
    e = {k: v for k, v in os.environ.items() if k not in SR.SWITCHES}
    e.update(env, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _QUERY], cwd=ROOT, env=e, timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])


def _slabs(shape, ws):
    B, HW, C = shape
    q, r = divmod(ws - 16384, B * (C // 64) * (C // 64 + 1) // 2 * 4096)
    assert r == 0
    return q


def test_out_of_range_values_are_clamped_on_the_host():
    """a negative NFS_C3*_BLOCKS is one block per tile (as 0); NFS_WINOGRAD_MIN_CH below 64 is 64 (a 32-channel layer
    stays direct); NFS_GRAM_CPS so small that the slabs would pass the reduce's fan-in of 256 is raised until they do not
    (1000 chunks: 4 per slab, 250 slabs; 257 chunks: 2 per slab, 129 slabs), and a value that keeps them below is taken
    as it is.  None of these values is ever launched."""
    d = _query({})
    assert (d["c3f"]["tiles"], d["c3d"]["tiles"]) == (1080, 720) and d["c3f"]["blocks"] < 1080 and d["c3d"]["blocks"] < 720
    assert d["narrow"] == "wg4_single" and d["thin"] == "direct"
    c = _query({"NFS_C3F_BLOCKS": "-3", "NFS_C3D_BLOCKS": "-1", "NFS_WINOGRAD_MIN_CH": "-5", "NFS_GRAM_CPS": "1"})
    assert c["c3f"]["blocks"] == 1080 and c["c3d"]["blocks"] == 720
    assert c["narrow"] == "wg4_single" and c["thin"] == "direct"
    shapes = ((1, 32000, 64), (2, 8224, 128), (1, 1000, 128))
    slabs = [_slabs(s, w) for s, w in zip(shapes, c["gram"])]
    assert slabs == [250, 129, 32], slabs
    assert all(n <= 256 for n in slabs)
