// svo_knobs.cpp -- the one parser of the SVO_* environment knobs (svo_knobs.hpp).  Host only, no HIP.
#include "svo_knobs.hpp"
#include <stdio.h>
#include <stdlib.h>

const char* knobs_env(const char* name) { return getenv(name); }

void knobs_read(Knobs* k, const char* (*get)(const char*))
{
    const auto num = [&](const char* name) { const char* e = get(name); return e ? atoi(e) : 0; };
    const auto zero = [&](const char* name) { const char* e = get(name); return e && atoi(e) == 0; };      // set, and to 0 (or to no number at all)
    k->debug_mode = num("SVO_DEBUG_MODE");
    k->rest_prio = num("SVO_REST_PRIO") & 3;
    { const char* e = get("SVO_TIMELINE"); k->timeline = e && e[0] == '1'; }
    k->ham_fp4 = !zero("SVO_HAM_FP4");
    { const int v = num("SVO_HAM_SPLITS"); k->ham_splits = v > 0 ? v : 0; }
    k->copy_prio_normal = zero("SVO_COPY_PRIO");
    { const int v = num("SVO_RS_C0"); k->rs_c0 = (v == SVO_RANSAC_CHUNK0 || v == SVO_RANSAC_CHUNK1 || v == SVO_RANSAC_FEW) ? v : 0; }
    k->rc_split[0] = RC16_NSPLIT0; k->rc_split[1] = k->rc_split[2] = 1;
    if (const char* e = get("SVO_RC_SPLIT")) {
        int v[3] = { 0, 0, 0 };
        const int n = sscanf(e, "%d,%d,%d", &v[0], &v[1], &v[2]);
        for (int i = 0; i < 3; i++) { const int x = i < n ? v[i] : (n > 0 ? v[n - 1] : 0); if (x >= 1 && x <= 8) k->rc_split[i] = x; }
    }
    { const int v = num("SVO_GN_NT"); k->gn_nt = (v == 256 || v == 384 || v == 512) ? v : 384; }
    { const int v = num("SVO_DESC_KPW"); k->desc_kpw = (v >= 1 && v <= 64) ? v : 8; }
    k->desc_tl = !zero("SVO_DESC_TL");
    k->nms_nt = num("SVO_NMS_NT");
}
