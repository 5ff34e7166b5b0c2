// fmj_stage_euler_commit.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// Euler, part 2 (after the freeze vote): commit qacc, qvel and the scalar joints' qpos; joint sensors on the last step.
// reads  frozen, isd, lane, my_qacc, nvel, hstep, pre_qd, d_scalar, d_qadr, d_act, last, CONS;  writes XV, QV, QP, steps_done
// a barrier follows in the kernel: the free-root update reads the committed QV
    if (isd && !frozen) {
      XV[lane] = my_qacc;
      QV[lane] = nvel;
      if (d_scalar) {
        const float pre_q = QP[d_qadr];
        QP[d_qadr] = pre_q + hstep * nvel;
        if (last) {
          float* s = glob(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * d_act.z;   // jointpos, jointvel, jointlimitfrc
          s[0] = pre_q; s[1] = pre_qd; if (!CONS) s[2] = 0.f;
        }
      }
    }
    if (!frozen) steps_done++;
