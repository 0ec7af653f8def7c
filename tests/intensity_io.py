"""File helpers shared by the intensity CLI tests: running the binaries,
writing a tile dataset, writing a match container in the [PIN-INTMATCH-IO]
layout and reading a coefficient dataset back."""

import json
import os
import struct
import subprocess

import numpy as np

from tests import intensity_ref as ir
from tests import n5util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("BS_BIN",
                     os.path.join(ROOT, "bigstitcher_spark_amd", "bin"))


def run(tool, *a, env=None):
    return subprocess.run([os.path.join(BIN, tool), *a],
                          capture_output=True, text=True, env=env)


def write_tiles(d, vols, affs):
    """dataset.n5 + dataset.xml of views placed by pure translations."""
    n5 = os.path.join(d, "dataset.n5")
    for i, vol in enumerate(vols):
        name = f"setup{i}/timepoint0/s0"
        n5util.write_dataset(n5, name, vol, (32, 32, 32))
        pth = os.path.join(n5, name, "attributes.json")
        with open(pth) as f:
            at = json.load(f)
        at["downsamplingFactors"] = [1, 1, 1]
        with open(pth, "w") as f:
            json.dump(at, f)
    xml = os.path.join(d, "dataset.xml")
    n5util.make_dataset_xml(xml, "dataset.n5", [
        dict(id=i, dims=v.shape[::-1], pos=tuple(float(t) for t in a[:, 3]))
        for i, (v, a) in enumerate(zip(vols, affs))])
    return xml


def write_matches(root, cg, pairs):
    """[PIN-INTMATCH-IO]: pairs = [((tp, setup), (tp, setup), records)]."""
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "attributes.json"), "w") as f:
        json.dump({"n5": "2.5.0", "coefficientsSize": list(cg)}, f)
    for va, vb, recs in pairs:
        ds = os.path.join(root, "matches", "tp%d_setup%d__tp%d_setup%d"
                          % (va + vb))
        os.makedirs(ds)
        n = len(recs)
        with open(os.path.join(ds, "attributes.json"), "w") as f:
            json.dump({"dimensions": [11, n], "blockSize": [11, max(n, 1)],
                       "dataType": "uint64",
                       "compression": {"type": "raw"}}, f)
        if n:
            arr = np.array([[r[k] for k in ir.FIELDS] for r in recs],
                           dtype=">u8")
            os.makedirs(os.path.join(ds, "0"))
            with open(os.path.join(ds, "0", "0"), "wb") as f:
                f.write(struct.pack(">HHII", 0, 2, 11, n) + arr.tobytes())


def read_coefficients(root, name):
    """float64 {gx, gy, gz, 2} dataset in one raw block -> (2, gz, gy, gx)."""
    with open(os.path.join(root, name, "attributes.json")) as f:
        at = json.load(f)
    assert at["dataType"] == "float64" and at["dimensions"][3] == 2
    assert at["blockSize"] == at["dimensions"]
    raw = open(os.path.join(root, name, "0", "0", "0", "0"), "rb").read()
    mode, nd = struct.unpack(">HH", raw[:4])
    dims = struct.unpack(">4I", raw[4:20])
    assert (mode, nd) == (0, 4) and list(dims) == at["dimensions"]
    return np.frombuffer(raw[20:], ">f8").astype(np.float64).reshape(
        dims[::-1])
