"""The opt-in fused launch of an fp64 context (fmj_step_fused_f64, BatchedPhysics(precision='fp64', fp64_fused=True)) as far as it can
be checked without a GPU: the entry point, its binding and its NULL check, the Python keyword, and the compiler's resource remarks for
the two instantiations of the fp64 step kernel (hipcc cross-compiles)."""
import ctypes
import inspect
import os
import re
import shutil

import pytest

from support_capi import lib as _lib, FMJ_ERR_ARG
from support_f64_interface import BUILD_FLAGS, lds_bytes, resource_remarks, within_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_exported_declared_and_bound():
    L, lib = _lib()
    assert hasattr(lib, 'fmj_step_fused_f64') and L.has('fmj_step_fused_f64')
    assert 'fmj_step_fused_f64' in L.OPTIONAL_IN_AB_BASE
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert re.search(r'int fmj_step_fused_f64\(fmj_ctx\* ctx, const fmj_data\* d, const fmj_fused_args\* args, const fmj_fused_ext\* ext', hdr)
    assert '#define FMJ_ABI_VERSION 6' in hdr
    assert ctypes.sizeof(L.CFusedExt) == 32 and ctypes.sizeof(L.CCreateOptions) == 16      # the structs it takes keep their layouts


def test_null_arguments_are_argument_errors_before_any_device_call():
    L, lib = _lib()
    a, cd = L.CFusedArgs(), L.CData()
    assert lib.fmj_step_fused_f64(None, ctypes.byref(cd), ctypes.byref(a), None, None) == FMJ_ERR_ARG
    assert 'NULL' in lib.fmj_last_error().decode()
    assert lib.fmj_step_fused_f64(None, None, None, None, None) == FMJ_ERR_ARG


def test_python_takes_fp64_fused_and_refuses_it_for_fp32_without_a_device():
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.model import salamander33
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_fused' in p and p['fp64_fused'].default is False
    with pytest.raises(ValueError, match='fp64_fused'):      # before any device use: no GPU is needed to get here
        BatchedPhysics(salamander33(), 2, precision='fp32', fp64_fused=True)
    m = salamander33()
    with pytest.raises(ValueError, match='fp64_fused'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, precision='fp32', fp64_fused=True)


def test_launch_fused_goes_through_the_new_entry_for_an_fp64_fused_physics(monkeypatch):
    """simulation._launch_fused keeps its four arguments and picks the entry by ``phys.fp64_fused`` (a stand-in library: no device)."""
    from types import SimpleNamespace
    from farms_mujoco_amd import _lib as L
    from farms_mujoco_amd.simulation import simulation as S
    monkeypatch.setattr(L, 'stream_ptr', lambda device: None)
    assert list(inspect.signature(S._launch_fused).parameters) == ['phys', 'cd', 'a', 'ext']
    calls = []
    fake = SimpleNamespace(fmj_step_fused=lambda *a: calls.append('fused') or 0, fmj_step_fused_ex=lambda *a: calls.append('ex') or 0,
                           fmj_step_fused_f64=lambda *a: calls.append(('f64', a[3] is None)) or 0)
    cd, a, ext = L.CData(), L.CFusedArgs(), L.CFusedExt(ctypes.sizeof(L.CFusedExt), 0)
    for fused64 in (False, True):
        phys = SimpleNamespace(_lib=fake, _ctx=None, device='cpu', fp64_fused=fused64)
        S._launch_fused(phys, cd, a, None)
        S._launch_fused(phys, cd, a, ext)
    assert calls == ['fused', 'ex', ('f64', True), ('f64', False)], calls
    S._launch_fused(SimpleNamespace(_lib=fake, _ctx=None, device='cpu'), cd, a, None)      # an object without the attribute: the old path
    assert calls[-1] == 'fused'


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_both_fp64_kernels_compile_without_scratch(tmp_path):
    """The fp64 translation unit with the flags of _lib.build() holds two kernels, the plain step and the fused loop; neither uses
    scratch or spills a VGPR, and the static LDS plus the largest dynamic request (ldsd_layout(128, 128, 129, 64) of fmj_f64.inc: the
    fused loop adds nothing to it) fits gfx950's 160 KB per workgroup."""
    from farms_mujoco_amd import _lib as L
    assert repr(BUILD_FLAGS)[:-1] in inspect.getsource(L.build) and "'-DFMJ_TU_F64'" in inspect.getsource(L.build), 'build() compiles with other flags: restate them in support_f64_interface'
    res = resource_remarks('-DFMJ_TU_F64', tmp_path)
    assert len(res) == 2 and all('f64' in k for k in res), sorted(res)
    layout = open(os.path.join(ROOT, 'farms_mujoco_amd', 'csrc', 'fmj_f64.inc')).read()
    layout = layout[layout.index('inline LdsLayoutD ldsd_layout'):layout.index('L.total_bytes = o * 8;')]
    assert layout.count('o +=') == 13, 'ldsd_layout changed: restate its sum in support_f64_interface.lds_bytes'      # the thirteen regions summed there
    within_resources(res, lds_bytes('plain', 128, 128, 129, 64))
