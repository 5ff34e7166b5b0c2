// fmj_stage_step_head.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// Head of a step: the launch arguments and the lane's indices laundered, the counters of iterations and sub-steps.
// reads  Mp, Ap, lane_outer, bl, dl, step, sub, itm
// defines lane, it, last, S_sub, full, nsub, nfull, nit, blo, dlo
    asm volatile("" : "+s"(Mp), "+s"(Ap));       // arguments are re-read from the kernarg segment in every step
    // per-lane LDS/global addresses are recomputed every step instead of being hoisted and spilled
    const int lane = opaque(lane_outer);
    const int it = A.iteration0 + itm;
    const bool last = step == A.n_steps - 1;
    const int S_sub = A.substeps;
    const bool full = sub == 0;
    const int nsub = sub + 1 >= S_sub ? 0 : sub + 1;           // the next physics step: its sub index, whether it is a full step,
    const bool nfull = nsub == 0;                               // and task.iteration as its before_step will see it: the reference
    const int nit = (nfull ? it + 1 : it) + ((nsub >= 1 && nsub >= S_sub - 1) ? 1 : 0);   // advances it after sub-step S - 2 (task.py:352-355)
    const int blo = opaque(bl), dlo = opaque(dl);
