"""The owner of a context's device and pinned memory (cl-rrt_amd/csrc/clrrt_devmem.hpp, no HIP) without a GPU: a
stand-alone host program (its own main, nothing loaded into Python) over counting malloc / free fakes, built with
-fsanitize=address,undefined.  The fakes' counters say "freed exactly once", the sanitizer's leak check at exit says
"nothing leaked".  The same program checks the guard bands (clrrt::MemGuard): one changed byte at the first and last byte
of either band is reported with its side and offset, by a check of the live blocks and at a free; a clean run reports
nothing; without a guard pointers pass through unchanged; a block keeps the guard it was allocated with."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cl-rrt_amd", "csrc")


def test_devmem_under_address_sanitizer(tmp_path):
    exe = tmp_path / "devmem_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "devmem_check.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and "failures 0" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_runtime_allocation_calls_only_where_the_policy_is_bound():
    """hipMalloc / hipHostMalloc / hipFree / hipHostFree appear in csrc once each: in clrrt_devmem_hip.hpp, where the
    owner's policy is bound to the runtime.  (A plain text count: a comment that spells one of the calls with its
    opening parenthesis trips it too -- reword the comment.)"""
    calls = ["hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree("]
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".hpp")):
            continue
        src = open(os.path.join(CSRC, name)).read()
        want = 1 if name == "clrrt_devmem_hip.hpp" else 0
        for call in calls:
            assert src.count(call) == want, (
                f"{name}: {src.count(call)} x '{call}', expected {want}: device and pinned memory goes through the "
                "context's owner (clrrt_devmem.hpp); comments count too")
