// PointNet++ on arbitrary rows: dgdm_pointnet2_forward and the plain 3-D forward dgdm_dyn3d_forward (no guidance handle).
#include "common.h"
#include "models.h"
#include <unordered_map>

using namespace dgdm;

namespace {

struct CloudGroup { std::vector<int> rows; };

// Runs the table pipeline for every distinct cloud among `rows` clouds and writes emb_dev [rows][256].
int pointnet_rows(DgdmDynamics *m, const float *xyz_dev /*[rows][3][N]*/, const int64_t *s1, const int64_t *s2, float *emb_dev, int rows,
                  int N, hipStream_t s) {
    DGDM_REQUIRE(N > 0 && N <= 1024, DGDM_EINVAL, "clouds of %d points unsupported (1..1024)", N);
    std::vector<float> host((size_t)rows * 3 * N);
    DGDM_HIP_CHECK(hipMemcpyAsync(host.data(), xyz_dev, host.size() * 4, hipMemcpyDeviceToHost, s));
    DGDM_HIP_CHECK(hipStreamSynchronize(s));
    // group bit-identical clouds (cond_fn hands 512 replicas of one cloud per call, diffusion.py:491)
    std::unordered_map<std::string, int> seen;
    std::vector<CloudGroup> groups;
    std::vector<int> rep;
    for (int r = 0; r < rows; ++r) {
        std::string key(reinterpret_cast<const char *>(host.data() + (size_t)r * 3 * N), (size_t)3 * N * 4);
        auto it = seen.find(key);
        int gid;
        if (it == seen.end()) {
            gid = (int)groups.size();
            seen.emplace(std::move(key), gid);
            groups.emplace_back();
            rep.push_back(r);
        } else {
            gid = it->second;
        }
        groups[gid].rows.push_back(r);
    }
    const PnWeights w = m->pn();
    DevBuf xyz, fps1, F1, U, Y, L2, Z, vlist, slotmap, starts, chains, out, crowded, clist, poff, pairs, prank;
    int rc;
    const PnWeights64 w64 = m->pn64();
    if ((rc = xyz.alloc((size_t)N * 12)) || (rc = fps1.alloc((size_t)N * 512 * 4)) || (rc = F1.alloc((size_t)N * 128 * 8)) || (rc = U.alloc((size_t)N * 128 * 8)) ||
        (rc = Y.alloc((size_t)N * N * 1024)) || (rc = chains.alloc(sizeof(XobjChain))) || (rc = crowded.alloc((size_t)N * 4)) ||
        (rc = clist.alloc((size_t)(N + 1) * 4)) || (rc = poff.alloc((size_t)(N + 1) * 4)) || (rc = pairs.alloc((size_t)N * N * 4)) ||
        (rc = prank.alloc((size_t)N * N * 2)))
        return rc;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const std::vector<int> &rws = groups[gi].rows;
        std::vector<float> pts((size_t)N * 3);
        const float *src = host.data() + (size_t)rep[gi] * 3 * N;
        for (int i = 0; i < N; ++i) { pts[3 * i] = src[i]; pts[3 * i + 1] = src[N + i]; pts[3 * i + 2] = src[2 * N + i]; }
        std::vector<int> slot_of(N, -1), vl, st(2 * rws.size());
        for (size_t k = 0; k < rws.size(); ++k) {
            const int64_t a = s1[rws[k]], b = s2[rws[k]];
            DGDM_REQUIRE(a >= 0 && a < N && b >= 0 && b < 512, DGDM_EINVAL, "FPS start out of range");
            if (slot_of[a] < 0) { slot_of[a] = (int)vl.size(); vl.push_back((int)a); }
            st[2 * k] = (int)a; st[2 * k + 1] = (int)b;
        }
        const int nv = (int)vl.size();
        if ((rc = xyz.upload(pts.data(), pts.size() * 4)) || (rc = vlist.upload(vl.data(), vl.size() * 4)) ||
            (rc = slotmap.upload(slot_of.data(), slot_of.size() * 4)) || (rc = starts.upload(st.data(), st.size() * 4)) ||
            (rc = L2.alloc((size_t)nv * N * 1024)) || (rc = Z.alloc((size_t)nv * N * 1024)) || (rc = out.alloc(rws.size() * 1024)))
            return rc;
        const float *x = xyz.as<float>();
        if ((rc = pn_fps_table(x, N, N, 512, fps1.as<int>(), nullptr, s))) return rc;
        if ((rc = pn_sa1_64(x, N, w.r1sq, w64, F1.as<double>(), s))) return rc;
        if ((rc = linear64(nullptr, F1.as<double>(), 128, w64.sa2_wf_t, w64.sa2_b0, nullptr, 1, U.as<double>(), nullptr, 128, N, 128, 128, ACT_NONE, s))) return rc;
        if ((rc = pn_crowd(x, N, w, crowded.as<int>(), clist.as<int>(), clist.as<int>() + N, poff.as<int>(), pairs.as<int>(), prank.as<short>(), s))) return rc;
        if ((rc = pn_pairs64(x, N, U.as<double>(), w64, pairs.as<int>(), poff.as<int>(), Y.as<float>(), s))) return rc;
        if ((rc = pn_l2(x, N, w, fps1.as<int>(), vlist.as<int>(), nv, Y.as<float>(), L2.as<float>(), clist.as<int>(), clist.as<int>() + N,
                        poff.as<int>(), prank.as<short>(), false, s))) return rc;
        if ((rc = pn_z64(x, N, nv, w64, L2.as<float>(), Z.as<float>(), clist.as<int>(), clist.as<int>() + N, s))) return rc;
        XobjChain ch{};
        ch.xyz = x; ch.fps1 = fps1.as<int>(); ch.slot_of_start = slotmap.as<int>(); ch.Z = Z.as<float>(); ch.fps2 = nullptr; ch.flags = nullptr; ch.crowded = crowded.as<int>(); ch.N = N;
        DGDM_HIP_CHECK(hipMemcpyAsync(chains.p, &ch, sizeof ch, hipMemcpyHostToDevice, s));
        XobjParams xp{};
        xp.chains = chains.as<XobjChain>(); xp.starts = starts.as<int>(); xp.xobj = out.as<float>(); xp.R = (int64_t)rws.size(); xp.total_rows = xp.R;
        if ((rc = pn_xobj(xp, false, s))) return rc;
        // scatter the group's rows back
        bool contiguous = true;
        for (size_t k = 1; k < rws.size(); ++k) contiguous = contiguous && rws[k] == rws[k - 1] + 1;
        if (contiguous) {
            DGDM_HIP_CHECK(hipMemcpyAsync(emb_dev + (size_t)rws[0] * 256, out.p, rws.size() * 1024, hipMemcpyDeviceToDevice, s));
        } else {
            for (size_t k = 0; k < rws.size(); ++k)
                DGDM_HIP_CHECK(hipMemcpyAsync(emb_dev + (size_t)rws[k] * 256, out.as<float>() + k * 256, 1024, hipMemcpyDeviceToDevice, s));
        }
        DGDM_HIP_CHECK(hipStreamSynchronize(s));     // per-group buffers are reused by the next group
    }
    return DGDM_OK;
}

}  // namespace

extern "C" int dgdm_pointnet2_forward(DgdmDynamics *m, const float *xyz_dev, const int64_t *start_sa1_host, const int64_t *start_sa2_host,
                                      float *emb_dev, int rows, int N, void *stream) {
    DGDM_REQUIRE(m && xyz_dev && start_sa1_host && start_sa2_host && emb_dev && rows >= 0, DGDM_EINVAL, "dgdm_pointnet2_forward: bad argument");
    if (m->kind != 3) { set_error("model type not supported: PointNet++ belongs to the 3-D model"); return DGDM_EMODE; }
    if (rows == 0) return DGDM_OK;
    return pointnet_rows(m, xyz_dev, start_sa1_host, start_sa2_host, emb_dev, rows, N, (hipStream_t)stream);
}

extern "C" int dgdm_dyn3d_forward(DgdmDynamics *m, const float *x_ctrl, const float *x_ori, const float *x_pos, const float *t,
                                  const float *xyz, const int64_t *start_sa1_host, const int64_t *start_sa2_host, float *logits, int rows,
                                  int N, void *stream) {
    DGDM_REQUIRE(m && x_ctrl && x_ori && x_pos && t && xyz && start_sa1_host && start_sa2_host && logits && rows >= 0, DGDM_EINVAL,
                 "dgdm_dyn3d_forward: bad argument");
    if (m->kind != 3) { set_error("model type not supported: dgdm_dyn3d_forward on a 2-D model"); return DGDM_EMODE; }
    if (rows == 0) return DGDM_OK;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // workspace: V, GENC [rows][256] | pose [rows][32] | tmp [rows][768] | z1 [rows][512] | xobj [rows][256]
    const size_t need = (size_t)rows * (256 + 256 + 32 + 768 + 512 + 256) * sizeof(float);
    if ((rc = m->ws.alloc(need))) return rc;
    float *V = m->ws.as<float>(), *genc = V + (size_t)rows * 256, *pose = genc + (size_t)rows * 256, *tmp = pose + (size_t)rows * 32,
          *z1 = tmp + (size_t)rows * 768, *xo = z1 + (size_t)rows * 512;
    if ((rc = pointnet_rows(m, xyz, start_sa1_host, start_sa2_host, xo, rows, N, s))) return rc;
    if ((rc = m->time_part(t, 0.f, tmp, z1, rows, s))) return rc;
    // x_ctrl[:, 1, :]  (profile_forward_3d.py:78): rows of length L at stride 3L, offset L
    if ((rc = m->gripper_forward(x_ctrl + m->L, 3 * m->L, V, genc, rows, s))) return rc;
    if ((rc = linear(genc, 256, m->blob.at(m->off.w1c_wt), nullptr, nullptr, 1, z1, 512, rows, 256, 512, ACT_NONE, true, s))) return rc;
    if ((rc = pose_embed(x_ori, x_pos, pose, rows, s))) return rc;
    if ((rc = linear(pose, 27, m->blob.at(m->off.w1p_wt), nullptr, nullptr, 1, z1, 512, rows, 27, 512, ACT_NONE, true, s))) return rc;
    TrunkParams p;
    m->fill_trunk(&p);
    p.Atab = z1; p.xobj = xo; p.logits = logits; p.C = rows; p.R = rows; p.xstride = rows; p.B = 1; p.tiles_per_b = 1; p.ntiles = (rows + 31) / 32;
    return trunk_launch(3, true, true, p, s);
}
