"""CPU: the kernels of the forward coefficient-probability update themselves (csrc/coef_update.hip compiled as plain C++ against
tests/emu/hip/hip_runtime.h, one thread per lane) against svt_hip_coef_update_picture: batches of pictures whose stream lengths sit on the
count kernel's pass and grid-stride boundaries, totals known to the "device" only, "old" tables of their own and the context's -- the
histogram, the partial sums, the searches, the reductions, the scan of the record places, the join and the refusals as the device runs
them, without a device.  Built twice: plain, and as the same stand-alone program under AddressSanitizer and UBSan with every buffer
allocated to exactly its size."""
import os
import subprocess
import tempfile

import boolcode_model as BM
import svt_testlib as T

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]
PICTURES = 6 + 3 + 6


def build(td, flags, name):
    emu, src = os.path.join(T.ROOT, "tests", "emu"), os.path.join(T.ROOT, "svt-vp9_amd")
    exe = os.path.join(td, name)
    cmd = ["g++"] + flags + ["-x", "c++", "-std=c++17", "-O1", "-w", f"-I{emu}", f"-I{os.path.join(src, 'csrc')}", os.path.join(emu, "coef_update", "coef_update_emu.cpp"),
                             "-x", "c", os.path.join(src, "host", "coef_update_host.c"), "-lpthread", "-o", exe]
    return exe if subprocess.run(cmd, capture_output=True).returncode == 0 else None


def test_kernel_text_on_the_cpu_equals_the_host_form():
    with tempfile.TemporaryDirectory() as td:
        plain, sanitized = build(td, [], "coef_update_emu"), build(td, SANITIZE, "coef_update_emu_san")
        assert plain
        tab = os.path.join(td, "tables.bin")
        with open(tab, "wb") as f:
            f.write(BM.tables()[1].tobytes())
        for exe in (plain, sanitized):
            if exe is None:
                continue
            r = subprocess.run([exe, tab], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and "bad 0" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
            assert r.stdout.count(" ok") == PICTURES and "sent 1111" in r.stdout and "sent 0000" in r.stdout
        print("sanitizers:", sanitized is not None)
