#!/usr/bin/env python3
"""Files written by the reference's OWN History and raw + XDMF2 writers (needs a checkout of the reference):

    python3 tests/golden/make_golden_reference_io.py <reference checkout>

-> tests/golden/reference_io.npz, read by tests/test_history_io.py.  Every file is stored as its bytes (uint8):
`vel_xmf` / `vel_raw`: a float32 node-centred field written as `a.xmf`; `p_xmf` / `p_raw`: the same values in float64,
cell-centred, written as `b.xmf`; `history_csv`: the train.csv of `history_rows`.  The inputs come from the test
module (`io_field`, `history_rows`)."""

import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

from test_history_io import history_rows, io_field  # noqa: E402


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main(reference):
    src = os.path.join(reference, "src", "odil")
    ref_io, ref_history = load(os.path.join(src, "io.py"), "ref_io"), load(os.path.join(src, "history.py"), "ref_history")
    d = tempfile.mkdtemp()
    u = io_field()
    ref_io.write_raw_with_xmf(u, os.path.join(d, "a.xmf"), spacing=(0.1, 0.2, 0.3), name="vel", cell=False)
    ref_io.write_raw_with_xmf(u.astype(np.float64), os.path.join(d, "b.xmf"), spacing=(1, 2, 3), name="p")
    history_rows(ref_history.History(csvpath=os.path.join(d, "train.csv"), warmup=1))
    read = lambda name: np.frombuffer(open(os.path.join(d, name), "rb").read(), dtype=np.uint8)
    data = dict(vel_xmf=read("a.xmf"), vel_raw=read("a.raw"), p_xmf=read("b.xmf"), p_raw=read("b.raw"),
                history_csv=read("train.csv"))
    path = os.path.join(HERE, "reference_io.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
