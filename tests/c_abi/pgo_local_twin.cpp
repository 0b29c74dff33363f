// TEST INFRASTRUCTURE — the host replay of the local-frame PGO solve (mv_pgo_solve_local).
//
// The two frame changes of Local_TwoFrame_PGO (Module/Optimization/TwoFramePGO/Optimizer.py:131-150) are mac-vo_amd/csrc/pgo_local_dev.h, the header
// the kernel's local instantiations include; this file includes that very header, moves the problem into the optimisation frame on the host, runs the
// existing twin's solve (pgo_twin.cpp, included as it is) on the moved tables and moves the result back.  The intermediate stages come back as well, so
// the CPU suite can pin each of them to the reference golden before the kernel reaches a GPU.
// Nothing in the product path builds, links or loads this file.
#include "pgo_twin.cpp"

#include "../../mac-vo_amd/csrc/pgo_local_dev.h"

// pgo_twin_solve's arguments + ref_pose [nprob,7] (T_o2w).  out_pose: the local-frame fp64 LM result; out_pose_f32 [nprob,7]: the fp32 world pose;
// stage outputs (each may be NULL): out_init_local [nprob,7] fp32 (T_c2o), out_pos_To [Ntot,3] fp32, out_cov_To [Ntot,9] fp64.
extern "C" int pgo_local_twin_solve(int nprob, const int32_t* offsets, int graph_type, const float* init_pose, const float* ref_pose,
                                    const float* intrinsics, const float* baseline, const float* pos_Tw, const double* cov_Tw,
                                    const float* pixel2_uv, const float* pixel2_d, const float* pixel2_disp, const float* pixel2_disp_cov,
                                    const float* pixel2_uv_cov, const double* obs2_covTc, const uint8_t* valid, int min_points,
                                    const mvLMParams* params, double* out_pose, double* out_info, float* out_pose_f32, int nw, int spec,
                                    float* out_init_local, float* out_pos_To, double* out_cov_To) {
    if (nprob < 0 || !params || !ref_pose) return 1;
    const int ntot = offsets[nprob];
    std::vector<float> init_l(7 * (size_t)nprob), pos_To(3 * (size_t)ntot);
    std::vector<double> cov_To(cov_Tw ? 9 * (size_t)ntot : 0);
    for (int p = 0; p < nprob; ++p) {
        LocalFrame f;
        local_frame(ref_pose + 7 * p, f);
        se3_mul_f32(f.T_w2o, init_pose + 7 * p, &init_l[7 * (size_t)p]);
        for (int i = offsets[p]; i < offsets[p + 1]; ++i) {
            local_point_f32(f, pos_Tw + 3 * (size_t)i, &pos_To[3 * (size_t)i]);
            if (cov_Tw) local_cov_f64(f, cov_Tw + 9 * (size_t)i, &cov_To[9 * (size_t)i]);
        }
    }
    const int rc = pgo_twin_solve(nprob, offsets, graph_type, init_l.data(), intrinsics, baseline, pos_To.data(), cov_Tw ? cov_To.data() : nullptr,
                                  pixel2_uv, pixel2_d, pixel2_disp, pixel2_disp_cov, pixel2_uv_cov, obs2_covTc, valid, min_points, params, out_pose,
                                  out_info, nullptr, nw, spec);
    if (rc) return rc;
    for (int p = 0; p < nprob && out_pose_f32; ++p) {
        float* w = out_pose_f32 + 7 * (size_t)p;
        if (out_info[4 * (size_t)p + 1] == 0.0) {   // below min_points (the LM loop never ran): the start pose as it is
            for (int k = 0; k < 7; ++k) w[k] = init_pose[7 * p + k];
        } else {
            const double* o = out_pose + 7 * (size_t)p;
            local_to_world_f32(ref_pose + 7 * p, o, o + 3, w);
        }
    }
    if (out_init_local) memcpy(out_init_local, init_l.data(), sizeof(float) * init_l.size());
    if (out_pos_To) memcpy(out_pos_To, pos_To.data(), sizeof(float) * pos_To.size());
    if (out_cov_To && cov_Tw) memcpy(out_cov_To, cov_To.data(), sizeof(double) * cov_To.size());
    return 0;
}
