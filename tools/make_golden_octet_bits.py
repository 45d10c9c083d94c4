"""Golden bit patterns of the eight-lane step kernels (tests/test_octet_bits_gpu.py): every case of
tests/octet_bits_cases.py run on the GPU, its state, records, flags and rare-path census written to
tests/golden/octet_bits.npz. A change to csrc/octet.hpp that is meant to leave every result as it is, is checked against a
fixture recorded from the library built BEFORE the change, on the same kind of GPU:

    UPKIE_HIP_LIBRARY=/path/to/libupkie_hip_before.so python tools/make_golden_octet_bits.py [out.npz]

The recorder refuses to write a fixture in which a case does not take the path it is named for (the census proves it).
With --census it only prints every case's counters."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np

from tests import octet_bits_cases as cases

args = [a for a in sys.argv[1:] if a != "--census"]
out_path = args[0] if args else os.path.join(ROOT, "tests", "golden", "octet_bits.npz")
arrays, missing = {}, []
for case in cases.CASES:
    out = cases.run_case(case)
    problem = cases.path_taken(case, out)
    print(f"{cases.case_id(case):24s} census {out['census'][:8].tolist()} episodes ended {int(out['episodes'][0])}"
          + ("" if problem is None else "   <-- path NOT taken"), flush=True)
    if problem is not None:
        missing.append(problem)
    for name, value in out.items():
        arrays[f"{cases.case_id(case)}/{name}"] = value
if "--census" in sys.argv[1:]:
    sys.exit(1 if missing else 0)
if missing:
    sys.exit("no fixture written:\n" + "\n".join(missing))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
np.savez_compressed(out_path, **arrays)
library = os.environ.get("UPKIE_HIP_LIBRARY", "the tree's own")
print(f"wrote {out_path}: {len(arrays)} arrays, {os.path.getsize(out_path)} bytes, library: {library}")
