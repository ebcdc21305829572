// C face of flowgnn_amd/csrc/gin_resident_launch.h for tests/test_gin_resident_select_cpu.py (ctypes).
#include "gin_resident_launch.h"

extern "C" {
// Each pointer argument of the selection as null / non-null.  Returns the instance's number; *fold, *enc and *refusal are the rest of the pick.
int grs_pick(int hout, int out, int head_u, int emb, int node_logits, int self_scale, int tb, int pooling, int tstride, int prof, int* fold,
             int* enc, const char** refusal) {
    static float f[5];
    fg::GinResidentLaunch a;
    a.hout = hout ? f : nullptr;
    a.out = out ? f : nullptr;
    a.head_u = head_u ? f : nullptr;
    a.emb = emb ? f : nullptr;
    a.node_logits = node_logits ? f : nullptr;
    a.self_scale = self_scale ? f : nullptr;
    a.tb = tb ? reinterpret_cast<const fg::GinTileBuild*>(f) : nullptr;  // (only compared with null)
    a.pooling = pooling;
    a.tstride = tstride;
    a.prof = prof != 0;
    const fg::GinResidentPick p = fg::gin_resident_pick(a);
    *fold = p.fold;
    *enc = p.enc;
    *refusal = p.refusal;
    return (int)p.instance;
}
}
