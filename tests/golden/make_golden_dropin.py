#!/usr/bin/env python3
"""What the reference's OWN operator functions trace to on this package's API (needs a checkout of the reference):

    python3 tests/golden/make_golden_dropin.py <reference checkout>

-> tests/golden/reference_operators_traced.npz, read by tests/test_reference_operators_dropin.py.  Every operator of
its CASES is loaded from the reference's example file by path, with `import odil` resolved to odil_amd
(`odil_alias`), handed unchanged to `odil_amd.Problem` on the restated example's domain and traced on the test's seeded
random state.  Stored per operator: the file and function it came from, the output names, every traced output
evaluated by the NumPy DAG interpreter, and the SHA-1 of every generated kernel source."""

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import test_reference_operators_dropin as t  # noqa: E402

import odil_amd  # noqa: E402


def main(reference):
    examples = os.path.join(reference, "examples")
    data = dict()
    for name, ref_file, opname, mine_name, argv in t.CASES:
        with pytest.MonkeyPatch.context() as mp:
            saved = t.odil_alias(mp)
            try:
                problem, state, arrays, nets = t.restated_problem(mine_name, argv)
                ref_operator = getattr(t.load_by_path(os.path.join(examples, ref_file), "reference_example_" + name), opname)
                assert os.path.abspath(ref_operator.__code__.co_filename).startswith(os.path.abspath(reference) + os.sep)
                ref_problem = odil_amd.Problem(ref_operator, problem.domain, problem.extra, tracers=dict(problem.tracers or {}))
                sources, names, values = t.traced_sources_and_values(ref_problem, state, arrays, nets)
            finally:
                odil_amd.util.g_log_file = saved
        data[name + "/ref_file"] = np.array(ref_file)
        data[name + "/opname"] = np.array(opname)
        data[name + "/names"] = np.array([n or "" for n in names])
        data[name + "/source_sha1"] = np.array([t.sha1(s) for s in sources])
        for k, v in enumerate(values):
            data["{}/value{}".format(name, k)] = v
        print(name, len(values), "outputs", len(sources), "kernel sources")
    path = os.path.join(HERE, "reference_operators_traced.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
