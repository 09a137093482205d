"""Device-only assembly of a csrc/ translation unit for gfx950, compiled once per session (a plain helper module): the ISA
hazard scan (tests/test_isa_hazards.py) and the plan-universe checks (tests/test_fwd_plan.py, tests/test_kv8_plan.py) read the
same file.  fp8_cache_kernels() is the kernel-symbol parser the fp8-KV-cache units share (tests/test_kv8_abi.py,
tests/test_qv8_abi.py, tests/test_kv8_plan.py)."""
import atexit
import functools
import os
import re
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


TYPES = {"DF16b": "bf16", "DF16_": "fp16"}


def kernel_bodies(unit):
    """[(mangled symbol, text of its .amdhsa_kernel block)] of every kernel in the device code of `unit`."""
    text = open(device_asm(unit)).read()
    return [(m.group(1), m.group(2))
            for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S)]


def fp8_cache_kernels(unit, kernel, params):
    """{(type, N, SOFTCAP): private segment bytes} of a forward unit over an fp8 KV cache, whose only kernels are the
    instantiations of fa::`kernel`<T, int N, bool SOFTCAP>(fa::`params`): ("fa_fwd_kv8_api.hip", "kv8_fwd_kernel", "PkParams"),
    ("fa_fwd_qv8_api.hip", "qv8_fwd_kernel", "QvParams").  Any other kernel symbol in the unit is an error."""
    out = {}
    for sym, body in kernel_bodies(unit):
        k = re.match(rf"_ZN2fa{len(kernel)}{kernel}I(DF16b|DF16_)Li(\d+)ELb([01])EEEvNS_{len(params)}{params}E$", sym)
        assert k, f"a kernel in {unit} that is no {kernel}: {sym}"
        key = (TYPES[k.group(1)], int(k.group(2)), bool(int(k.group(3))))
        assert key not in out
        out[key] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    return out
