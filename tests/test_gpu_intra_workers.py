"""The intra pass packs four independent 64-lane workers into each workgroup (csrc/intra_kernel.hip).  Whatever the number of workers --
fewer than a workgroup holds, a last workgroup that is partly empty, more workers than there are tickets -- every picture has to come out
byte-equal to the oracle chain: reconstruction, coefficients, eob map (and everything else the checks of test_gpu_intra.py /
test_gpu_encdec.py compare).

The failure this file is there for is a HANG: workers of one workgroup loop different numbers of times, so a single workgroup barrier left
in the kernel would stop it for good, and a hung kernel cannot be interrupted from inside its process.  The cases therefore run in ONE
child process that serves them one by one; the test waits for each answer under a timeout, kills the child when none comes, and every
later case then fails at once without starting anything more on the GPU."""
import functools
import os
import select
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

START_TIMEOUT_S = 300   # interpreter + torch + context + the first launch's code-object load
CASE_TIMEOUT_S = 60     # a case is a few small pictures and their oracle: a second or two

DEFAULT, MORE_THAN_TICKETS = 0, 100000
WORKERS = [1, 2, 3, 4, 5, 7, 128, DEFAULT, MORE_THAN_TICKETS]
# "sizes": every block size, 32x32 and 4x4 included (20 x 12 cells); "odd": 9 x 5 = 45 cells, 135 tickets -- no multiple of four;
# "mixed": the intra blocks of an inter picture (13 x 9 cells), through the batch entry
KINDS = ["sizes", "odd", "mixed"]


def _serve():
    """child: reads `<kind> <workers>` lines, answers `OK` or `FAIL <text>`"""
    import ctypes as C
    import traceback
    import torch
    torch.cuda.init()           # before the library pulls in the system's HIP runtime (tests/conftest.py)
    import svt_testlib as T
    import test_gpu_encdec as TE
    import test_gpu_intra as TI
    B = T.B
    lib = B.load()
    ctx = C.c_void_p()
    B.check(lib.svt_hip_ctx_create(C.byref(ctx), 0))
    TE.make_inputs = functools.lru_cache(maxsize=None)(TE.make_inputs)   # (the ME oracle of the mixed picture: once, not per worker count)
    inter = dict(enc_mode=8, tune=1, temporal_layer_index=0, is_used_as_reference=1, recon_file=0, loop_filter=1)
    run = {
        "sizes": lambda: TI.check(ctx, 320, 192, 3, 200, TI.KEY, sizes=(4, 8, 16, 32)),
        "odd": lambda: TI.check(ctx, 136, 72, 32, 120, TI.KEY, sizes=(4, 8, 16, 32)),
        "mixed": lambda: TE.test_intra_blocks_inside_inter_pictures(ctx, 200, 136, 2, 120, inter),
    }
    print("READY", flush=True)
    for line in sys.stdin:
        kind, n = line.split()
        try:
            B.check(lib.svt_hip_ctx_set_intra_workgroups(ctx, int(n)))
            run[kind]()
            print("OK", flush=True)
        except BaseException:  # noqa: BLE001 -- an assertion of the checks included: its text is the answer
            print("FAIL " + traceback.format_exc().replace("\n", " | ")[-1500:], flush=True)
    lib.svt_hip_ctx_destroy(ctx)


class Child:
    def __init__(self):
        self.dead = None
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        self.expect("READY", START_TIMEOUT_S)

    def readline(self, timeout):
        if not select.select([self.p.stdout], [], [], timeout)[0]:
            self.p.kill()
            self.dead = f"no answer within {timeout} s: the child was killed (a hung intra pass?)"
            pytest.fail(self.dead)
        line = self.p.stdout.readline()
        if not line:
            self.dead = f"the child ended (exit status {self.p.wait()})"
            pytest.fail(self.dead)
        return line.strip()

    def expect(self, what, timeout):
        # (the runtime may print lines of its own before ours)
        for _ in range(50):
            line = self.readline(timeout)
            if line == what or line.startswith("FAIL"):
                return line
        pytest.fail(f"no `{what}` from the child")

    def case(self, kind, n):
        if self.dead:
            pytest.fail("not run: " + self.dead)
        self.p.stdin.write(f"{kind} {n}\n")
        self.p.stdin.flush()
        return self.expect("OK", CASE_TIMEOUT_S)

    def close(self):
        if self.p.poll() is None:
            try:
                self.p.stdin.close()
                self.p.wait(timeout=60)
            except Exception:
                self.p.kill()
                self.p.wait()


@pytest.fixture(scope="module")
def child():
    c = Child()
    yield c
    c.close()


@pytest.mark.parametrize("n", WORKERS)
@pytest.mark.parametrize("kind", KINDS)
def test_any_number_of_packed_workers_gives_the_oracles_picture(child, kind, n):
    assert child.case(kind, n) == "OK"


if __name__ == "__main__" and sys.argv[1:] == ["--serve"]:
    _serve()
