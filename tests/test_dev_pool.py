"""csrc/dev_pool.h, the one owner of what a context allocates, on the CPU: oracle/dev_pool_check.cpp
drives the header with a counting backend that fails the k-th request, for every k from 1 to the
number of requests its script makes (single allocations of each kind, a group of four, a
grow-and-retire sequence, releases of null / unknown / already released pointers, destruction).  For
every k it asserts that a failed group leaves its pointers null and the live count where it was,
that no handle is released twice, and that nothing is live once the pool is destroyed.  The program
is built with the address and undefined-behaviour sanitizers and run as a child process."""
import re
import subprocess
from pathlib import Path


def test_pool_under_every_failing_request(oracle):
    exe = Path(oracle.__file__).resolve().parent / "build" / "dev_pool_check"
    assert exe.exists(), "oracle/Makefile builds dev_pool_check"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr                     # a sanitizer report goes there
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    m = re.fullmatch(r"dev_pool_check ok: requests=(\d+) runs=(\d+) failures_injected=(\d+) handles=(\d+) "
                     r"double_releases=(\d+) leaked=(\d+)", lines[0])
    assert m, lines[0]
    requests, runs, injected, handles, twice, leaked = map(int, m.groups())
    # 6 single requests (device, pinned, two events, two streams), the group's 4, three grows of 2
    assert requests == 16
    assert runs == requests + 1 and injected == requests  # every k from 1 to the number of requests, and none
    assert handles > requests
    assert twice == 0 and leaked == 0
