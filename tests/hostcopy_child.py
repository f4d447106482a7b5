"""The child process of tests/test_hostcopy_gpu.py -- TEST INFRASTRUCTURE ONLY, not collected by pytest.

    python hostcopy_child.py <k> <bytes> [<bytes> ...]

The staged device-to-host copy (csrc/mm_hostcopy.hip) sizes its copy threads by the CPUs the process may run on, read on
every call but fixed for this process HERE: before the library is imported the child narrows its own affinity to the first
k CPUs of the mask it was given (never wider), so k = 1 takes the plain copy and k = 2, 6, 16 take 1, 3 and 8 copy threads.
For each byte count it makes the host run of test_hostcopy_gpu.host_run (integer-state MH into a caller-owned buffer between
two guards) and prints `<bytes> <cpus> <sha256 of the result> <guards intact: 1 | 0>`.  Any exception -- a HIP error status
among them -- ends the process with a non-zero exit code at once: nothing further runs on the device."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(k, byte_counts):
    given = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, given[:k])
    cpus = len(os.sched_getaffinity(0))
    assert cpus == min(k, len(given))

    import test_hostcopy_gpu as T  # imports the library

    for nbytes in byte_counts:
        dest = T.Dest(nbytes)
        T.host_run(nbytes, dest)
        print(nbytes, cpus, hashlib.sha256(dest.payload()).hexdigest(), int(dest.guards_intact()), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]), [int(a) for a in sys.argv[2:]])
