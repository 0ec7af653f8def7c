"""CPU tests of `solver -s IP` (reference Solver.java:434-670): links from
the corresponding interest points stored in interestpoints.n5
([PIN-IPCORR], csrc/host/bs_ipio.h), written here by hand so that no GPU
is involved."""

import json
import os
import struct

import numpy as np

from tests import n5util
from tests.test_cli_host import BIN, run
from tests.test_cli_solver import model_translations


def _write_2d(root, name, arr, dtype):
    """(N, rows) array -> N5 dataset [rows, N], one [rows, 300000] block."""
    n, rows = arr.shape
    ds = os.path.join(root, name)
    os.makedirs(os.path.join(ds, "0"), exist_ok=True)
    with open(os.path.join(ds, "attributes.json"), "w") as f:
        json.dump({"dimensions": [rows, n], "blockSize": [rows, 300000],
                   "dataType": dtype,
                   "compression": {"type": "zstd", "level": 3}}, f)
    be = {"uint64": ">u8", "float64": ">f8"}[dtype]
    body = n5util.zstd_compress(np.ascontiguousarray(arr, be).tobytes())
    with open(os.path.join(ds, "0", "0"), "wb") as f:
        f.write(struct.pack(">HHII", 0, 2, rows, n) + body)


def _attrs(root, group, **kv):
    os.makedirs(os.path.join(root, group), exist_ok=True)
    with open(os.path.join(root, group, "attributes.json"), "w") as f:
        json.dump(kv, f)


def _dataset(tmp_path, pos, points, corrs, label="beads"):
    """pos: XML position per setup; points: per setup (N,3) view-local
    locations; corrs: per setup list of (own id, other id, other setup)."""
    d = str(tmp_path)
    xml = os.path.join(d, "dataset.xml")
    n5util.make_dataset_xml(xml, "input.n5", [
        dict(id=i, dims=(64, 64, 64), pos=tuple(p))
        for i, p in enumerate(pos)])
    ipn5 = os.path.join(d, "interestpoints.n5")
    _attrs(ipn5, "", n5="4.0.0")
    vip = "  <ViewInterestPoints>\n"
    for i, loc in enumerate(points):
        g = f"tpId_0_viewSetupId_{i}/{label}"
        _attrs(ipn5, g + "/interestpoints", **{
            "pointcloud": "1.0.0", "type": "list", "list version": "1.0.0"})
        ids = np.arange(len(loc), dtype=np.uint64)[:, None]
        _write_2d(ipn5, g + "/interestpoints/id", ids, "uint64")
        _write_2d(ipn5, g + "/interestpoints/loc",
                  np.asarray(loc, np.float64), "float64")
        others = sorted({o for _, _, o in corrs[i]})
        idmap = {f"0,{o},{label}": k for k, o in enumerate(others)}
        _attrs(ipn5, g + "/correspondences", correspondences="1.0.0",
               idMap=idmap)
        if corrs[i]:
            rows = np.array([[a, b, idmap[f"0,{o},{label}"]]
                             for a, b, o in corrs[i]], np.uint64)
            _write_2d(ipn5, g + "/correspondences/data", rows, "uint64")
        vip += (f'    <ViewInterestPointsFile timepoint="0" setup="{i}" '
                f'label="{label}" params="test">{g}'
                "</ViewInterestPointsFile>\n")
    vip += "  </ViewInterestPoints>\n"
    text = open(xml).read()
    open(xml, "w").write(text.replace("</SpimData>", vip + "</SpimData>"))
    return xml


def _chain(tmp_path):
    """Three views in a row; views 1 and 2 are registered off by e1, e2.
    10 matches link 0-1, 30 link 1-2, 5 wrong-by-(3,0,0) ones link 0-2."""
    rng = np.random.default_rng(3)
    true = np.array([[0.0, 0, 0], [40.0, 0, 0], [80.0, 0, 0]])
    e = np.array([[0.0, 0, 0], [2.5, -1.5, 1.0], [-1.0, 0.5, 2.0]])
    world = rng.uniform(0, 60, (45, 3)) + np.array([30.0, 0, 0])
    pts = [world - true[i] for i in range(3)]   # view-local, all 45 in each
    corrs = [[], [], []]
    for k in range(10):
        corrs[0].append((k, k, 1))
        corrs[1].append((k, k, 0))
    for k in range(10, 40):
        corrs[1].append((k, k, 2))
        corrs[2].append((k, k, 1))
    pts[2] = pts[2].copy()
    pts[2][40:] += np.array([3.0, 0, 0])
    for k in range(40, 45):
        corrs[0].append((k, k, 2))
        corrs[2].append((k, k, 0))
    return _dataset(tmp_path, true + e, pts, corrs), true, e


def _expected(true, e, w01, w12, w02):
    # minimise sum w ((t_b - t_a) - d)^2 with t_0 = 0; d = pA - pB (world)
    d01, d12 = -e[1], e[1] - e[2]
    d02 = -e[2] - np.array([3.0, 0, 0])
    A = np.array([[w01 + w12, -w12], [-w12, w12 + w02]])
    rhs = np.stack([w01 * d01 - w12 * d12, w12 * d12 + w02 * d02])
    return np.linalg.solve(A, rhs)


def test_solver_ip_chain(tmp_path):
    xml, true, e = _chain(tmp_path)
    r = run([os.path.join(BIN, "solver"), "-x", xml, "-s", "IP", "-l",
             "beads"])
    assert r.returncode == 0, r.stderr + r.stdout
    assert "3 interest point links from 45 matches" in r.stdout
    t = model_translations(xml)
    want = _expected(true, e, 10.0, 30.0, 5.0)   # weight = match count
    assert np.allclose(t[0], true[0], atol=1e-12)
    assert np.allclose(t[1], true[1] + e[1] + want[0], atol=1e-9)
    assert np.allclose(t[2], true[2] + e[2] + want[1], atol=1e-9)
    # the count weighting matters on this graph
    assert np.abs(want - _expected(true, e, 1.0, 1.0, 1.0)).max() > 0.1
    text = open(xml).read()
    assert text.count("Interest Point Transform") == 3
    assert "Stitching Transform" not in text


def test_solver_ip_dry_run(tmp_path):
    xml, true, e = _chain(tmp_path)
    r = run([os.path.join(BIN, "solver"), "-x", xml, "-s", "IP", "-l",
             "beads", "--fixedViews", "0,1", "--dryRun"])
    assert r.returncode == 0, r.stderr + r.stdout
    assert model_translations(xml)[1][0] == 42.5      # --dryRun: untouched


def test_solver_ip_label_weight_and_errors(tmp_path):
    xml, true, e = _chain(tmp_path)
    before = open(xml).read()
    bin_ = os.path.join(BIN, "solver")
    r = run([bin_, "-x", xml, "-s", "IP"])
    assert r.returncode == 2 and "-l" in r.stderr
    r = run([bin_, "-x", xml, "-s", "IP", "-l", "beads", "-tm", "RIGID"])
    assert r.returncode == 2 and "not supported" in r.stderr
    r = run([bin_, "-x", xml, "-s", "BOTH", "-l", "beads"])
    assert r.returncode == 2
    r = run([bin_, "-x", xml, "-s", "IP", "-l", "beads", "-lw", "1", "-lw",
             "2"])
    assert r.returncode == 2
    r = run([bin_, "-x", xml, "-s", "IP", "-l", "nuclei"])
    assert r.returncode == 1 and "nothing to solve" in r.stderr
    assert open(xml).read() == before
    # a uniform label weight scales every link alike: same solution
    r = run([bin_, "-x", xml, "-s", "IP", "-l", "beads", "-lw", "2.5"])
    assert r.returncode == 0, r.stderr + r.stdout
    t = model_translations(xml)
    want = _expected(true, e, 10.0, 30.0, 5.0)
    assert np.allclose(t[1], true[1] + e[1] + want[0], atol=1e-9)
