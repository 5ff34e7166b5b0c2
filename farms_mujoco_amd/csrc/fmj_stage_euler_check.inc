// fmj_stage_euler_check.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// Euler, part 1: the new velocity and the warn tests; the kernel's freeze vote follows.
// reads  my_qacc, isd, lane, QV, QP;  updates warn
// defines hstep, pre_qd, nvel
    // ---- semi-implicit Euler (mj_Euler with implicit joint damping)
    const float hstep = A.integrate ? M.h : 0.f;     // fmj_forward: mj_forward only
    const float pre_qd = isd ? QV[lane] : 0.f;
    const float nvel = pre_qd + hstep * my_qacc;
    if (isd) {
      if (!(fabsf(my_qacc) <= 1e10f)) warn |= FMJ_WARN_BADQACC;      // mj_checkAcc
      if (!(fabsf(nvel) <= 1e10f)) warn |= FMJ_WARN_BADQVEL;
      // the root position this step would commit is tested BEFORE anything is committed (the translational dofs of a free root are
      // dofs 0..2 at qpos 0..2): a step that raises BADQPOS leaves qpos, qvel and time exactly at the previous step's values
      if (M.root_free && lane < 3 && A.integrate && !(fabsf(QP[lane] + M.h * nvel) <= 1e10f)) warn |= FMJ_WARN_BADQPOS;
    }
