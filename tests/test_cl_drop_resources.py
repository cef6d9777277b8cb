"""Compile-time guard of the channel-last last-level kernels (csrc/lfgc_wavelet_cl.hip): no instantiation, DROP or not,
spills a register or uses scratch.  The DROP adjoint gets there by forming its per-band uniform offsets anew in every z
step instead of letting the compiler keep them across the loop; a compiler that decides otherwise shows up here, not as
a slower kernel.  Needs hipcc (cross-compiles for gfx950), no GPU."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resource_usage():
    from latent_feature_grid_compression_amd import build
    src = os.path.join(build.CSRC, 'lfgc_wavelet_cl.hip')
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc()] + build.FLAGS + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', src,
                                                '-o', os.path.join(tmp, 'cl.o')]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r'(VGPRs|AGPRs|SGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)', line)
        if m and cur is not None:
            cur[m.group(1).split(' [')[0]] = int(m.group(2))
    return kernels


def test_no_instantiation_spills():
    kernels = resource_usage()
    cl = {k: v for k, v in kernels.items() if 'idwt_cl_kernel' in k or 'analysis_cl_kernel' in k}
    # synthesis: 3 channel widths x 2 store policies x 2 bases x DROP; adjoint: 2 widths x 2 tile sizes x 2 bases x DROP
    assert len(cl) == 24 + 16, sorted(cl)
    drop = [k for k in cl if k.split('EEvNS')[0].endswith('Lb1E')]
    assert len(drop) == 20, drop
    for name, use in sorted(cl.items()):
        assert use['VGPRs Spill'] == 0 and use['SGPRs Spill'] == 0 and use['ScratchSize'] == 0, (name, use)
    # the occupancy the host's workgroups-per-CU arguments (pick_zchunk) assume: 4 waves per SIMD for every synthesis
    # build and for the 64-cell adjoint, 5 for the db2 DROP adjoint with 32-cell tiles
    for name, use in cl.items():
        assert use['Occupancy'] >= 4, (name, use)
        if re.search(r'analysis_cl_kernelILi\d+ELi1ELi2ELb1E', name):
            assert use['Occupancy'] >= 5, (name, use)
