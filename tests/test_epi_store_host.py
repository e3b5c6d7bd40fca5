"""CPU: build-level guard for the buffer-store epilogue of the fp32 GEMM tiles (store_acc_buf, csrc/gemm_f32.hip).

Every gemm_f32_kernel instantiation now carries two epilogues (the buffer stores and, for what they do not serve, store_acc). The
second one must cost no resident wave: csrc/gemm_f32.hip is compiled for gfx950 with the project's flags and
-Rpass-analysis=kernel-resource-usage, and the waves per SIMD of the instantiations the fp32 bench step runs are pinned at the
values the same command reports for the commit before the epilogue (listed in profiles/epi_store_kernel_stats.md)."""
import os
import re
import subprocess

import __graft_entry__ as ge

# mangled template arguments <AL, BL, N64, STAGES> -> waves per SIMD before the buffer-store epilogue
WAVES = {
    "gemm_f32_kernelINS_16ConvAStripLoaderILb1EEENS_8KCLoaderILb0EEELb0ELi1E": 3,      # conv2 / conv3 forward
    "gemm_f32_kernelINS_16ConvAStripLoaderILb0EEENS_8KCLoaderILb0EEELb0ELi1E": 3,      # conv3 data gradient
    "gemm_f32_kernelINS_11ConvALoaderILb0EEENS_8KCLoaderILb0EEELb1ELi1E": 4,           # conv2 data gradient (128 x 64 tile)
    "gemm_f32_kernelINS_8MCLoaderILb0EEENS_16ConvWgradBLoaderILb1ELb0EEELb0ELi1E": 4,  # conv2 / conv3 weight gradient
    "gemm_f32_kernelINS_8KCLoaderILb1EEENS1_ILb0EEELb0ELi2E": 2,                       # linear5 forward
    "gemm_f32_kernelINS_8KCLoaderILb0EEENS_8MCLoaderILb0EEELb0ELi2E": 2,               # linear5 dX
    "gemm_f32_kernelINS_8KCLoaderILb0EEES2_Lb0ELi2E": 2,                               # the fusion MLP's forward
    "gemm_f32_kernelINS_8MCLoaderILb0EEES2_Lb0ELi1E": 4,                               # the fusion MLP's weight gradients
    "gemm_f32_epi_kernelINS_8MCLoaderILb0EEENS1_ILb1EEELi1ELi1E": 4,                   # linear5 weight gradient + Adam
}


def test_the_bench_step_kernels_keep_their_waves_per_simd(tmp_path):
    src = os.path.join(ge.CSRC, "gemm_f32.hip")
    r = subprocess.run([ge.HIPCC, *ge.FLAGS, "-I" + os.path.join(ge.ROOT, "include"), "--cuda-device-only", "-c", src, "-o", str(tmp_path / "g.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    waves = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(names) == len(waves) and len(names) >= 10
    for key, want in WAVES.items():
        got = [w for n, w in zip(names, waves) if key in n]
        print(f"{key}: waves/SIMD {got} (pinned {want})")
        assert got == [want], f"{key}: waves per SIMD {got}, the parent's build has {want}"
