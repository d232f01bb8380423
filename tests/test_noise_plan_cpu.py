"""The launch planner and the noisy collision, on a host: plan.cpp is plain C++, compiled here and asked how a run of a scalar lattice
is split with the noise off and on.  The size rule with noise (profiles/scalar_bench.txt, the noise column; DESIGN.md section 17: k_ad_tile4
with its noise plane in LDS against the noisy k_ad_step, both families, 256^2 ... 8192^2): PERIODIC, the tiles were 1.33-2.15 x faster at
all six sizes -- the noiseless range stands; OPEN, 2.10 x and 1.39 x at 256^2 and 512^2 and 0.97-1.03 x from 1024^2 up -- tiles below
1024^2 only.  Sizes outside 256^2 ... 8192^2 were never measured and stay on k_ad_step, as without noise.  An explicit variant decides
as before."""
import os
import shutil
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <stdio.h>
#include "plan.h"
int main()
{
    PlanInputs s;
    s.p = lb_params();
    s.p.semantics = LB_SEM_DIFFUSION; s.p.omega = 1.f;
    const int sizes[8] = {64, 256, 512, 1024, 2048, 4096, 8192, 16384};
    const int bcs[2] = {LB_BC_PERIODIC, LB_BC_OPEN};
    for (int noisy = 0; noisy < 2; ++noisy)
        for (int bc : bcs) {
            s.noisy = noisy != 0; s.p.bc_mode = bc; s.variant = -1;
            for (int n : sizes) {
                s.p.nx = s.p.ny = s.p.local_ny = s.H = n; s.pitch = n; s.plane = n; s.rowp = 9LL * n;
                int d[8];
                const int c = plan_launches(&s, 6, d, 8);
                char name[256];
                hot_kernel(&s, name, sizeof(name));
                printf("%d%d%d%c", scalar_use_tiles(&s) ? 1 : 0, steps_per_launch(&s), c, name[5]);       /* k_ad_[s]tep / k_ad_[t]ile4 */
                printf(n == 16384 ? "\n" : " ");
            }
        }
    /* an explicit variant decides, noisy or not */
    s.noisy = true; s.p.nx = s.p.ny = s.p.local_ny = s.H = 1024;
    s.variant = 1 << 9;
    printf("%d %d\n", scalar_use_tiles(&s) ? 1 : 0, steps_per_launch(&s));
    s.variant = 0;
    printf("%d %d\n", scalar_use_tiles(&s) ? 1 : 0, steps_per_launch(&s));
    return 0;
}
"""

TILES, STEP = "143t", "016s"       # tiles chosen: 4 steps per launch, 6 steps = 4 + 1 + 1; k_ad_step: six launches


def test_automatic_choice_of_a_noisy_handle_follows_its_own_size_rule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    csrc = os.path.join(ROOT, "2d-lb_amd", "csrc")
    (tmp_path / "drv.cpp").write_text(DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-Wall", "-I" + csrc, str(tmp_path / "drv.cpp"), os.path.join(csrc, "plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode().splitlines()
    plain = " ".join([STEP] + [TILES] * 6 + [STEP])             # the size rule without noise: 256^2 ... 8192^2 (test_scalar_cpu.py)
    noisy_open = " ".join([STEP] + [TILES] * 2 + [STEP] * 5)     # 256^2, 512^2
    assert out[0] == out[1] == plain, out[:2]
    assert out[2] == plain, out[2]                               # noisy, PERIODIC
    assert out[3] == noisy_open, out[3]
    assert out[4] == "1 4" and out[5] == "0 1"
