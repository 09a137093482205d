"""Device-only assembly of a csrc/ translation unit for gfx950, compiled once per session (a plain helper module): the ISA
hazard scan (tests/test_isa_hazards.py) and the plan-universe check (tests/test_fwd_plan.py) read the same file."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flash_attention_annotated_amd", "csrc")


@functools.lru_cache(maxsize=None)
def device_asm(unit):
    """Path of `unit` (e.g. "fa_fwd_api.hip") compiled with the library's flags to device assembly."""
    tmp = tempfile.mkdtemp(prefix="fa_asm_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, os.path.splitext(unit)[0] + ".s")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, unit), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return out
