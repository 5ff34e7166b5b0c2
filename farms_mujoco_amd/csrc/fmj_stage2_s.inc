// fmj_stage2_s.inc - step stage shared by the two-env kernel (fmj_dual2.inc) and the two-env constraint kernel (fmj_cons2.inc): a block
// of statements on the including kernel's locals.  STAGE2_REC is the kernel's stride of the CD / F records in floats.
// S: subtree sums as prefix-sum differences inside the half (fp64 DPP scans, see fmj_hip.hip).
// reads  mass, dcom, c_ipos (.w = subtree mass), lastl (last lane of the body's subtree), iw, fbody, sl, nb;  writes CI, F
      const double dm = (double)mass;
      const double dx = (double)dcom.x, dy = (double)dcom.y, dz = (double)dcom.z;
      const double ms = (double)c_ipos.w;
      const double px = half_subtree_sum_f64(dm * dx, lastl), py = half_subtree_sum_f64(dm * dy, lastl), pz = half_subtree_sum_f64(dm * dz, lastl);
      const double minv = ms > 0.0 ? rcp_f64_nr(ms) : 0.0;
      const double ex = px * minv, ey = py * minv, ez = pz * minv;
      // two scans at a time: their dependent DPP chains interleave (the fences keep it to two: sixteen fp64 inputs formed
      // up front would cost ~50 VGPRs)
#define SCAN2(ra_, rb_, ea_, eb_, post_a_, post_b_) do { \
        double pa_ = (ea_), pb_ = (eb_); \
        const double xa_ = pa_, xb_ = pb_; \
        pa_ += dpp_f64<0x111, 0xF>(pa_); pb_ += dpp_f64<0x111, 0xF>(pb_); \
        pa_ += dpp_f64<0x112, 0xF>(pa_); pb_ += dpp_f64<0x112, 0xF>(pb_); \
        pa_ += dpp_f64<0x114, 0xF>(pa_); pb_ += dpp_f64<0x114, 0xF>(pb_); \
        pa_ += dpp_f64<0x118, 0xF>(pa_); pb_ += dpp_f64<0x118, 0xF>(pb_); \
        pa_ += dpp_f64<0x142, 0xA>(pa_); pb_ += dpp_f64<0x142, 0xA>(pb_); \
        const double sa_ = lane_gather_f64(pa_, lastl) - pa_ + xa_, sb_ = lane_gather_f64(pb_, lastl) - pb_ + xb_; \
        ra_ = pinf((float)(sa_ + (post_a_))); rb_ = pinf((float)(sb_ + (post_b_))); } while (0)
      float i0, i1, i2, i3, i4, i5;
      SCAN2(i0, i1, (double)pinf(iw[0]) + dm * (dy * dy + dz * dz), (double)pinf(iw[1]) + dm * (dx * dx + dz * dz), -ms * (ey * ey + ez * ez), -ms * (ex * ex + ez * ez));
      SCAN2(i2, i3, (double)pinf(iw[2]) + dm * (dx * dx + dy * dy), (double)pinf(iw[3]) - dm * dx * dy, -ms * (ex * ex + ey * ey), ms * ex * ey);
      SCAN2(i4, i5, (double)pinf(iw[4]) - dm * dx * dz, (double)pinf(iw[5]) - dm * dy * dz, ms * ex * ez, ms * ey * ez);
      s6 fs;
      SCAN2(fs.r.x, fs.r.y, (double)pinf(fbody.r.x), (double)pinf(fbody.r.y), 0.0, 0.0);
      SCAN2(fs.r.z, fs.l.x, (double)pinf(fbody.r.z), (double)pinf(fbody.l.x), 0.0, 0.0);
      SCAN2(fs.l.y, fs.l.z, (double)pinf(fbody.l.y), (double)pinf(fbody.l.z), 0.0, 0.0);
#undef SCAN2
      if (sl < nb) {
        // subtree CoM relative to the tree CoM (what the H entries need), subtree mass
        *(float4*)(CI + sl * 12) = make_float4(i0, i1, i2, i3);
        *(float4*)(CI + sl * 12 + 4) = make_float4(i4, i5, (float)ex, (float)ey);
        *(float2*)(CI + sl * 12 + 8) = make_float2((float)ez, (float)ms);
        lds_put6(F + sl * STAGE2_REC, fs);
      }
