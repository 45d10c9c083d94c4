"""What the reference's OWN compiled low-pass filter (upkie/cpp/utils/low_pass_filter.h, through oracle/_ref) returns
on the inputs of tests/test_reference_cpp.py: the filter's outputs bit for bit (float64), whether it threw FilterError,
and the four filter chains of the spine observers over a seeded servo sequence. The test compares the oracle's
restatements against this file wherever it runs, the reference tree or no.

Output: tests/golden/reference_low_pass_filter.npz (committed). Build container only (oracle/_ref is built from the
reference's sources):

    python tools/make_golden_filter.py
"""

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "reference_low_pass_filter.npz")
# (cutoff_period, dt) around the Nyquist guard of low_pass_filter.h:22-30
NYQUIST_CASES = ((0.01, 0.005), (0.0100001, 0.005), (0.2, 0.1), (0.008, 0.005))


def main() -> None:
    from oracle import oracle as O

    ref = O.ref_lib()
    if ref is None:
        sys.exit("oracle/_ref was not built: this needs the reference's sources")
    threw = C.c_int(0)

    def f(prev, cutoff, new, dt):
        out = ref.ref_low_pass_filter(prev, cutoff, new, dt, C.byref(threw))
        return out, threw.value

    # single calls over the filter's domain
    rng = np.random.default_rng(0)
    calls = np.empty((500, 4))
    for i in range(len(calls)):
        prev, new = rng.uniform(-10, 10, 2)
        dt = float(rng.uniform(1e-4, 0.02))
        calls[i] = prev, new, dt, float(rng.uniform(2.0 * dt * 1.0001, 2.0))
    outputs, threw_calls = zip(*(f(prev, cutoff, new, dt) for prev, new, dt, cutoff in calls))
    assert not any(threw_calls)
    nyquist_threw = np.array([f(0.0, cutoff, 1.0, dt)[1] for cutoff, dt in NYQUIST_CASES], dtype=np.int32)

    # WheelContact::observe's three filters (WheelContact.cpp:26-31) and the upper-leg torque filter
    # (FloorContact.cpp:87-90) over a seeded servo sequence, dt = 1 ms
    dt = 1e-3
    rng = np.random.default_rng(1)
    servo_velocity, servo_torque, chains = np.empty((400, 6)), np.empty((400, 6)), np.empty((400, 4))
    v = a = t = leg = 0.0
    for k in range(400):
        servo_velocity[k] = rng.uniform(-5, 5, 6)
        servo_torque[k] = rng.uniform(-2, 2, 6)
        prev = v
        v = f(v, 0.2, servo_velocity[k, 2], dt)[0]
        a = f(a, 0.2, abs((v - prev) / dt), dt)[0]
        t = f(t, 0.2, abs(servo_torque[k, 2]), dt)[0]
        leg = f(leg, 0.01, float(np.sqrt(np.sum(servo_torque[k, [0, 1, 3, 4]] ** 2))), dt)[0]
        chains[k] = v, a, t, leg
    np.savez(OUT, calls=calls, outputs=np.array(outputs), nyquist_cases=np.array(NYQUIST_CASES), nyquist_threw=nyquist_threw,
             servo_velocity=servo_velocity, servo_torque=servo_torque, chains=chains)
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
