"""Models past one wavefront (up to 128 bodies / dofs, no constraints) go to the two-wave step kernel (csrc/fmj_wide.inc); what stays
refused is refused with a message that names its limit.  fmj_create validates a model before it looks for a device, so these run
without a GPU.  The last test compiles the two-wave kernel for gfx950 and reads the compiler's resource remarks (hipcc cross-compiles)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from support_capi import create as _create, no_gpu as _no_gpu, FMJ_ERR_UNSUPPORTED, FMJ_ERR_NODEVICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_model_sizes():
    """The models the two-wave kernel exists for: the table of the feature's issue, from the model compiler."""
    from farms_mujoco_amd.model import centipede
    m = centipede(20, 25)
    assert (m.nbody, m.nv, m.nu) == (107, 111, 105)
    m = centipede(12, 50)
    assert (m.nbody, m.nv, m.nu) == (100, 104, 98)


def test_unconstrained_model_past_64_reaches_the_device_lookup():
    """centipede(20, 25) (107 bodies, nv 111) passes every model check: on a machine without a GPU it is FMJ_ERR_NODEVICE, not
    FMJ_ERR_UNSUPPORTED; on a machine with one it is created."""
    from farms_mujoco_amd.model import centipede
    rc, msg = _create(centipede(20, 25))
    if _no_gpu():
        assert rc == FMJ_ERR_NODEVICE, (rc, msg)
    else:
        assert rc == 0, (rc, msg)


def test_limits_on_a_wide_model_are_refused():
    from farms_mujoco_amd.model import centipede
    m = centipede(20, 25)
    m.jnt_limited = np.ones_like(m.jnt_limited)
    m.jnt_range = np.tile([-1.0, 1.0], (m.njnt, 1)).astype(float)
    rc, msg = _create(m)
    assert rc == FMJ_ERR_UNSUPPORTED and '64' in msg and 'wavefront' in msg, (rc, msg)


def test_more_than_128_dofs_is_refused():
    from farms_mujoco_amd.model import centipede
    m = centipede(25, 30)
    assert m.nv == 136
    rc, msg = _create(m)
    assert rc == FMJ_ERR_UNSUPPORTED and '128' in msg, (rc, msg)


def test_rk4_on_a_wide_model_is_refused():
    from farms_mujoco_amd.model import centipede, INTEGRATORS
    m = centipede(20, 25)
    m.integrator = INTEGRATORS['rk4']
    rc, msg = _create(m)
    assert rc == FMJ_ERR_UNSUPPORTED and 'RK4' in msg and '64' in msg, (rc, msg)


def test_long_dof_chain_is_refused_by_the_chain_check():
    """eel(70): nbody 72, nv 76 fit two waves, but its dof chain of 76 does not fit a register row."""
    from farms_mujoco_amd.model import eel
    rc, msg = _create(eel(n_joints=70))
    assert rc == FMJ_ERR_UNSUPPORTED and 'chain longer than 64' in msg and 'wavefront' in msg, (rc, msg)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
@pytest.mark.parametrize('maxd', [32, 64])
def test_wide_kernel_compiles_without_scratch(tmp_path, maxd):
    """Every instantiation of the two-wave kernel keeps its register row in registers: no VGPR spill, no scratch (flags of
    _lib.build(), remarks parsed as scripts/kres.py does); the DPP reads of its wave reductions obey the wait-state rule
    (scripts/dpp_hazards.py on the -S listing)."""
    src = os.path.join(ROOT, 'farms_mujoco_amd', 'csrc', 'fmj_hip.hip')
    flags = ['--offload-arch=gfx950', '-O3', '-fno-slp-vectorize', '-mllvm', '-pragma-unroll-threshold=131072', '-fPIC', f'-DFMJ_TU_WIDE={maxd}']
    r = subprocess.run(['hipcc'] + flags + ['-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path/'kw.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kern, res = None, {}
    for line in r.stderr.splitlines():
        mm = re.search(r'remark:\s+(.*?) \[-Rpass', line)
        if not mm:
            continue
        t = mm.group(1).strip()
        if t.startswith('Function Name:'):
            kern = t.split(':', 1)[1].strip()
            res[kern] = {}
        elif kern:
            k, v = t.split(':', 1)
            res[kern][k.strip()] = v.strip()
    wide = {k: v for k, v in res.items() if 'fmj_step_wide_kernel' in k}
    assert sorted(wide) == sorted(f'_Z20fmj_step_wide_kernelILb{f}ELi{maxd}EEv8DevModel8StepArgs' for f in (0, 1)), sorted(res)
    for k, v in wide.items():
        assert v['ScratchSize [bytes/lane]'] == '0' and v['VGPRs Spill'] == '0', (k, v)
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import dpp_hazards
    out = str(tmp_path/'kw.s')
    subprocess.check_call(['hipcc'] + flags + ['-S', '--cuda-device-only', '-o', out, src])
    n, bad = dpp_hazards.check(out)
    assert n > 0 and not bad, (n, bad[:5])
