// Test tool: what mvs_postprocess_face_infos (csrc/oneshot.hip) does on its temporary context -- dc_postprocess, then phases 2 and 3 --
// on a context the CALLER owns, so that a test can switch on "profile" and "stats" and read the table with mvs_ctx_costs_download.
// The lists arrive with every face's list reversed, as dc_postprocess takes them.  Links the product library; nothing of the product uses it.
#include "../../mvs-texturing_amd/csrc/ctx.h"

extern "C" mvs_status test_dc_postprocess_on(mvs_ctx* ctx, uint32_t n_faces, uint32_t n_views, const uint32_t* info_ptr, const uint16_t* view_rev, const float* q_rev,
                                             const float* col_rev, const mvs_settings* settings, mvs_dc_stats* stats) {
    MVS_CTX_API_BEGIN
    mvs::dc_postprocess(ctx, n_faces, n_views, info_ptr, view_rev, q_rev, col_rev, settings);
    mvs::dc_phase2(ctx);
    mvs::dc_phase3(ctx, stats);
    MVS_API_END
}
