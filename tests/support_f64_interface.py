"""What the fp64 interface tests (test_f64_*_interface.py, test_f64_create_matrix.py) share: fmj_create_ex2 through ctypes, the LDS
bytes of each kernel family (csrc/fmj_f64.inc), and the compiler's resource remarks for one translation unit.  Nothing here needs a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

from support_capi import lib, no_gpu, F64, FMJ_ERR_NODEVICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'farms_mujoco_amd', 'csrc', 'fmj_hip.hip')
LIMITS, RK4, CONTACTS, TERRAIN = 1, 8, 32, 128      # FMJ_CREATE_F64_* of include/fmj.h
F64_CT, F64_TN = 33, 3      # doubles of LDS per contact: the contacts kernels' record, the terrain kernels' normal past it (csrc/fmj_f64.inc)
BUILD_FLAGS = ['--offload-arch=gfx950', '-O3', '-fno-slp-vectorize', '-mllvm', '-pragma-unroll-threshold=131072', '-fPIC']      # _lib.build()


def create_ex2(m, precision=F64, flags=LIMITS, size=None, ext=True):
    """fmj_create_ex2(m, 4 envs, options, ext) and destroy: the return code, the message, the precision and the solver the context reports."""
    L, so = lib()
    c = m.as_c(); ctx = ctypes.c_void_p()
    opts = L.CCreateOptions(ctypes.sizeof(L.CCreateOptions), precision, 0, 0)
    e = L.CCreateExt(ctypes.sizeof(L.CCreateExt) if size is None else size, flags)
    rc = so.fmj_create_ex2(ctypes.byref(c), 4, 0, ctypes.byref(opts), ctypes.byref(e) if ext else None, ctypes.byref(ctx))
    prec = solver = None
    if rc == 0:
        prec = so.fmj_precision(ctx); solver = L.ints(so.fmj_solver_info, ctx)
        so.fmj_destroy(ctx)
    return rc, so.fmj_last_error().decode(), prec, solver


def accepted(rc, msg, prec):
    """Every model check passed: without a GPU the first thing that fails is the device lookup."""
    return rc == FMJ_ERR_NODEVICE if no_gpu() else (rc == 0 and prec == F64)


def limited_eel48():
    from farms_mujoco_amd.model import eel
    m = eel(n_joints=48)
    m.jnt_limited = np.ones_like(m.jnt_limited)
    m.jnt_range = np.tile([-0.1, 0.1], (m.njnt, 1)).astype(float)
    return m


def lds_bytes(family, nb, nv, nq, rs, max_contacts=0, nu=0):
    """The dynamic LDS of a kernel family of csrc/fmj_f64.inc: ldsd_layout for 'plain'; F64_LIMITS_LDS_DOUBLES = 20 doubles more for
    'limits' (ldsd_total_bytes) and every family below; F64_RK4_LDS_DOUBLES(nu) = 2 nu + 12 rows of a double per lane for 'rk4' (its
    LIMITS builds); F64_CT doubles per contact for 'contacts' (ldsd_contacts_bytes), F64_TN more for 'terrain' (ldsd_terrain_bytes)."""
    extra = {'plain': 0, 'limits': 20, 'rk4': 20 + 2*nu + 12*128, 'contacts': 20 + F64_CT*max_contacts,
             'terrain': 20 + (F64_CT + F64_TN)*max_contacts}[family]
    return 8*(((nq + 1) & ~1) + 2*((nv + 1) & ~1) + 2*128*8 + nv*6 + nb*(10 + 10 + 6 + 6 + 4) + nv*rs + 128 + 4 + extra)


def resource_remarks(tu_define, tmp_path):
    """Compile the translation unit ``tu_define`` (-DFMJ_TU_F64[=n]) with the flags of _lib.build() and return the compiler's
    kernel-resource-usage remarks: {mangled kernel name: {remark: value}}."""
    r = subprocess.run(['hipcc'] + BUILD_FLAGS + [tu_define, '-Rpass-analysis=kernel-resource-usage', '-c', SRC, '-o', str(tmp_path/'kf64.o')],
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
    return res


def within_resources(kernels, dyn):
    """No scratch, no VGPR spill, and static + dynamic LDS within gfx950's 160 KB per workgroup, for every kernel of ``kernels``."""
    for k, v in kernels.items():
        assert v['ScratchSize [bytes/lane]'] == '0' and v['VGPRs Spill'] == '0', (k, v)
        assert int(v['LDS Size [bytes/block]']) + dyn <= 160*1024, (k, v, dyn)
