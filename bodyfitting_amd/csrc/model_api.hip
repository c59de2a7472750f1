// Host side of libbodyfit: the body model (bf_model_create).  The descriptor is checked before anything is allocated (check_desc),
// the host tables are derived from it without a HIP call (derive_tables), then each table struct - FitTab, MeshTab, KpIO, the
// sub-models - uploads what it points at and takes the pointers (fill_*).
#include "bf_host.h"
#include "dev_route.h"
#include "fit_kernels.h"
#include "mesh_kernels.h"
#include <memory>
#include <numeric>


namespace {

// posedirs rows are padded to a multiple of 128 bytes: a tile's 96 columns are 384 bytes, and with the natural pitch (SMPL: 82,680 B)
// every slice straddled a fourth line that the neighbouring tile's workgroup - usually on another XCD - fetched again (counter
// traffic 1.30 x the algorithmic bytes in rounds 2-4)
int pd_pitch_of(int cols) { return (cols + 31) & ~31; }
int n_all_joints(const bf_model_desc *d) { return d->n_joints + d->n_selector + d->n_extra + (d->model_kind == 1 ? d->n_lmk_static + d->n_lmk_dynamic : 0); }
size_t n_dyn(const bf_model_desc *d) { return (size_t)d->n_dyn_rows * d->n_lmk_dynamic; }

int check_desc(const bf_model_desc *d) {
    if (d->n_verts <= 0 || d->n_joints < 2 || d->n_joints > 64 || d->n_betas <= 0 || d->n_betas > 12)
        return fail(BF_ERR_UNSUPPORTED, "bf_model_create: need 2..64 joints and 1..12 betas");
    if (d->gmm_components != BF_GMM_M || d->gmm_dim != BF_GMM_D)
        return fail(BF_ERR_UNSUPPORTED, "bf_model_create: the GMM prior must be 8 components x 69 dims");
    if (d->n_loss_joints <= 0 || d->n_loss_joints > 192 || d->n_loss_joints > d->n_joint_map)
        return fail(BF_ERR_UNSUPPORTED, "bf_model_create: 1..192 loss joints supported");
    const bool smplx = d->model_kind == 1;
    const int nv = d->n_verts, nj = d->n_joints, n_all = n_all_joints(d);
    if (d->n_extra > 32 || n_all > 256) return fail(BF_ERR_UNSUPPORTED, "bf_model_create: too many auxiliary joints");
    if (smplx && (d->n_joints != 55 || d->n_hand_pca <= 0 || d->n_hand_pca > 6 || !d->pose_mean || !d->left_hand_components ||
                  !d->right_hand_components || !d->faces || d->n_faces <= 0 || !d->lmk_faces_idx || !d->lmk_bary_coords ||
                  (d->n_lmk_dynamic > 0 && (!d->dynamic_lmk_faces_idx || !d->dynamic_lmk_bary_coords || d->n_dyn_rows < 79)) ||
                  d->neck_joint < 0 || d->neck_joint >= 55))
        return fail(BF_ERR_INVALID, "bf_model_create: incomplete SMPL-X description");
    if (d->parents[0] != -1) return fail(BF_ERR_INVALID, "bf_model_create: parents[0] must be -1");
    for (int j = 1; j < nj; ++j)
        if (d->parents[j] < 0 || d->parents[j] >= j) return fail(BF_ERR_INVALID, "bf_model_create: parents[i] must be in [0,i)");
    for (int i = 0; i < d->n_selector; ++i)
        if (d->selector_ids[i] < 0 || d->selector_ids[i] >= nv) return fail(BF_ERR_INVALID, "bf_model_create: selector id out of range");
    for (int i = 0; i < d->n_joint_map; ++i)
        if (d->joint_map[i] < 0 || d->joint_map[i] >= n_all) return fail(BF_ERR_INVALID, "bf_model_create: joint_map entry out of range");
    for (int k = 0; k < d->n_loss_joints && d->n_loss_joints <= 32; ++k)       // (a dense keypoint loss reads every kind of joint)
        if (d->joint_map[k] >= nj + d->n_selector) return fail(BF_ERR_UNSUPPORTED, "bf_model_create: a loss joint maps to an extra-regressor joint");
    std::vector<int> n_children(nj, 0);
    for (int j = 1; j < nj; ++j)
        if (++n_children[d->parents[j]] > 6) return fail(BF_ERR_UNSUPPORTED, "bf_model_create: a joint has more than 6 children");
    for (int i = 0; d->faces && i < d->n_faces * 3; ++i)
        if (d->faces[i] < 0 || d->faces[i] >= nv) return fail(BF_ERR_INVALID, "bf_model_create: face index out of range");
    for (int i = 0; smplx && i < d->n_lmk_static; ++i)
        if (d->lmk_faces_idx[i] < 0 || d->lmk_faces_idx[i] >= d->n_faces) return fail(BF_ERR_INVALID, "bf_model_create: landmark face out of range");
    for (size_t i = 0; smplx && i < n_dyn(d); ++i)
        if (d->dynamic_lmk_faces_idx[i] < 0 || d->dynamic_lmk_faces_idx[i] >= d->n_faces)
            return fail(BF_ERR_INVALID, "bf_model_create: dynamic landmark face out of range");
    return BF_OK;
}

// ---- host tables: functions of the descriptor, no HIP call -----------------------------------------------------------------------

// kinematic tree: depth levels, children lists, descendant masks, depth-first order
struct Tree { int n_levels = 1; std::vector<int> depth, level_start, level_joints, child_start, child_list, dfs_order, dfs_last; std::vector<unsigned long long> desc; };
Tree derive_tree(const bf_model_desc *d) {
    const int nj = d->n_joints;
    const int *parents = d->parents;
    Tree t;
    t.depth.assign(nj, 0);
    for (int j = 1; j < nj; ++j) { t.depth[j] = t.depth[parents[j]] + 1; t.n_levels = std::max(t.n_levels, t.depth[j] + 1); }
    for (int l = 0; l < t.n_levels; ++l) {
        t.level_start.push_back((int)t.level_joints.size());
        for (int j = 0; j < nj; ++j) if (t.depth[j] == l) t.level_joints.push_back(j);
    }
    t.level_start.push_back((int)t.level_joints.size());
    for (int p = 0; p < nj; ++p) {
        t.child_start.push_back((int)t.child_list.size());
        for (int j = 1; j < nj; ++j) if (parents[j] == p) t.child_list.push_back(j);
    }
    t.child_start.push_back((int)t.child_list.size());
    t.desc.assign(nj, 0ull);
    for (int j = nj - 1; j >= 1; --j) t.desc[parents[j]] |= t.desc[j] | (1ull << j);
    // depth-first order (children in index order): a subtree is a contiguous run of positions, so subtree sums are
    // differences of a prefix sum
    std::vector<int> stack{0};
    while (!stack.empty()) {
        int j = stack.back(); stack.pop_back();
        t.dfs_order.push_back(j);
        for (int c = nj - 1; c >= 1; --c) if (parents[c] == j) stack.push_back(c);
    }
    for (int i = 0; i < nj; ++i) t.dfs_last.push_back(i + __builtin_popcountll(t.desc[t.dfs_order[i]]));
    return t;
}
// pre-contracted joint regressor: float64 accumulation row by row over the non-zero weights, rounded once; the differences to the
// parent joint are float64 differences
struct Regressor { std::vector<float> Jt, Jd, Jtrel, Jdrel; };
Regressor contract_regressor(const bf_model_desc *d) {
    const int nv = d->n_verts, nj = d->n_joints, nb = d->n_betas, w3 = 3 + 3 * nb;
    std::vector<double> acc((size_t)nj * w3, 0.0);        // per joint: [Jt 3 | Jd 3 x nb]
    for (int j = 0; j < nj; ++j) {
        double *a = acc.data() + (size_t)j * w3;
        for (int v = 0; v < nv; ++v) {
            double w = d->j_regressor[(size_t)j * nv + v];
            if (w == 0.0) continue;
            for (int k = 0; k < 3; ++k) {
                a[k] += w * d->v_template[(size_t)v * 3 + k];
                const float *sd = d->shapedirs + ((size_t)v * 3 + k) * nb;
                for (int l = 0; l < nb; ++l) a[3 + k * nb + l] += w * sd[l];
            }
        }
    }
    Regressor r;
    for (int j = 0; j < nj; ++j) {
        const double *a = acc.data() + (size_t)j * w3, *p = j > 0 ? acc.data() + (size_t)d->parents[j] * w3 : nullptr;
        for (int e = 0; e < w3; ++e) {
            (e < 3 ? r.Jt : r.Jd).push_back((float)a[e]);
            (e < 3 ? r.Jtrel : r.Jdrel).push_back((float)(p ? a[e] - p[e] : a[e]));
        }
    }
    return r;
}
// The model's per-vertex tables gathered for a list of vertices (row i = vertex verts[i]): posedirs rows at `pd_pitch` floats, zero
// padded; sparse skinning rows of `nnz` entries (0: none) - the first nnz non-zero weights in joint order, zero padded; max_nnz: the
// most non-zero weights of one of the vertices.
struct Gather { std::vector<float> vt, sd, pd, lw, jx, zw; std::vector<int> zj; int max_nnz = 0; };
Gather gather_vertices(const bf_model_desc *d, const std::vector<int> &verts, int pd_pitch, int nnz) {
    const int nv = d->n_verts, nj = d->n_joints, nb = d->n_betas, npf = 9 * (nj - 1), ne = std::max(d->n_extra, 0);
    const size_t n = verts.size();
    Gather g;
    g.vt.resize(n * 3); g.sd.resize(n * 3 * nb); g.pd.assign((size_t)npf * pd_pitch, 0.f); g.lw.resize(n * nj); g.jx.resize((size_t)ne * n);
    g.zj.assign(n * std::max(nnz, 1), 0); g.zw.assign(n * std::max(nnz, 1), 0.f);
    for (size_t i = 0; i < n; ++i) {
        const int v = verts[i];
        for (int k = 0; k < 3; ++k) {
            g.vt[i * 3 + k] = d->v_template[(size_t)v * 3 + k];
            for (int l = 0; l < nb; ++l) g.sd[(i * 3 + k) * nb + l] = d->shapedirs[((size_t)v * 3 + k) * nb + l];
            for (int p = 0; p < npf; ++p) g.pd[(size_t)p * pd_pitch + i * 3 + k] = d->posedirs[(size_t)p * 3 * nv + (size_t)v * 3 + k];
        }
        int c = 0;
        for (int j = 0; j < nj; ++j) {
            const float w = g.lw[i * nj + j] = d->lbs_weights[(size_t)v * nj + j];
            if (w != 0.f && c < nnz) { g.zj[i * nnz + c] = j; g.zw[i * nnz + c] = w; }
            c += w != 0.f;
        }
        g.max_nnz = std::max(g.max_nnz, c);
        for (int e = 0; e < ne; ++e) g.jx[(size_t)e * n + i] = d->j_regressor_extra[(size_t)e * nv + v];
    }
    return g;
}
// the landmarks' corner vertices (MeshTab::lmk_fv / dyn_fv) looked up once in `faces` (the model's, or a sub-model's re-indexed copy)
struct Corners { std::vector<int> sfv, dfv; };
Corners landmark_corners(const bf_model_desc *d, const int *faces) {
    Corners c;
    for (int i = 0; i < d->n_lmk_static; ++i)
        for (int k = 0; k < 3; ++k) c.sfv.push_back(faces[(size_t)d->lmk_faces_idx[i] * 3 + k]);
    for (size_t i = 0; i < n_dyn(d); ++i)
        for (int k = 0; k < 3; ++k) c.dfv.push_back(faces[(size_t)d->dynamic_lmk_faces_idx[i] * 3 + k]);
    if (c.dfv.empty()) c.dfv.push_back(0);
    return c;
}
// GMM: symmetrised precisions and -log of the merged weights (prior.py:188-189); lane-major register images of Psym for the fit
// kernel (coalesced one-off load)
struct GmmImages { std::vector<float> means, psym, logw, plane, ptail; };
GmmImages gmm_images(const bf_model_desc *d) {
    const int M = BF_GMM_M, D = BF_GMM_D;
    const float *P = d->gmm_precisions;
    GmmImages g;
    g.means.assign(d->gmm_means, d->gmm_means + (size_t)M * D);
    g.psym.resize((size_t)M * D * D);
    for (int c = 0; c < M; ++c) {
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                g.psym[((size_t)c * D + i) * D + j] = (float)(0.5 * ((double)P[((size_t)c * D + i) * D + j] + (double)P[((size_t)c * D + j) * D + i]));
        g.logw.push_back((float)(-std::log((double)d->gmm_nll_weights[c])));
    }
    g.plane.assign((size_t)M * BF_GMM_LD * 64, 0.f); g.ptail.assign((size_t)4 * 12 * 64, 0.f);
    for (int c = 0; c < M; ++c)
        for (int j = 0; j < D; ++j)
            for (int l = 0; l < 64; ++l) g.plane[((size_t)c * BF_GMM_LD + j) * 64 + l] = g.psym[((size_t)c * D + l) * D + j];
    for (int w = 0; w < 4; ++w)
        for (int l = 0; l < 60; ++l) {
            int comp = l < 30 ? 2 * w : 2 * w + 1, row = 64 + (l % 30) / 6, col = 12 * (l % 6);
            for (int e = 0; e < 12; ++e)
                if (col + e < D) g.ptail[((size_t)w * 12 + e) * 64 + l] = g.psym[((size_t)comp * D + row) * D + col + e];
        }
    return g;
}
// The fit's scalar fields (sizes, the parameter vector's layout) for `nl` routed loss joints and `ns` selector vertices.
FitTab fit_sizes(const bf_model_desc *d, int nl, int ns, int n_levels) {
    const bool smplx = d->model_kind == 1;
    const int nj = d->n_joints, nb = d->n_betas, n_body = smplx ? 21 : nj - 1, n_pca = smplx ? d->n_hand_pca : 0;
    FitTab T{};
    T.nj = nj; T.nb = nb; T.npf = 9 * (nj - 1); T.ns = ns; T.nl = nl; T.n_levels = n_levels;
    T.np = smplx ? 3 + 1 + 63 + nb + 3 + 3 + 3 + 2 * n_pca : 3 + 1 + 3 * (nj - 1) + nb + 3; T.nbp = 3 * n_body;
    T.off_pose = 4; T.off_beta = 4 + 3 * n_body; T.off_orient = T.off_beta + nb;
    T.n_pca = n_pca; T.off_lh = T.off_orient + 9; T.off_rh = T.off_lh + n_pca; T.kp_dense = d->n_loss_joints > 32;
    return T;
}
// parameter routing: where each joint's theta comes from (FitTab::th_kind / th_off), what each parameter's gradient is (p_kind / p_a / p_b)
struct Routing { std::vector<int> th_kind, th_off, p_kind, p_a, p_b; };
Routing route_params(const FitTab &T) {
    const int off_leye = T.off_orient + 3, off_reye = T.off_orient + 6, n_body = T.nbp / 3;
    Routing r{std::vector<int>(T.nj, 0), std::vector<int>(T.nj, 0), std::vector<int>(T.np, 0), std::vector<int>(T.np, 0), std::vector<int>(T.np, -1)};
    std::vector<int> &thk = r.th_kind, &tho = r.th_off, &pk = r.p_kind, &pa = r.p_a, &pb = r.p_b;
    for (int j = 0; j < T.nj; ++j) {
        if (j == 0) { thk[j] = 0; tho[j] = T.off_orient; }
        else if (j <= n_body) { thk[j] = 0; tho[j] = T.off_pose + 3 * (j - 1); }
        else if (j == 22) { thk[j] = 1; }
        else if (j == 23) { thk[j] = 0; tho[j] = off_leye; }
        else if (j == 24) { thk[j] = 0; tho[j] = off_reye; }
        else if (j < 40) { thk[j] = 2; tho[j] = j - 25; }
        else { thk[j] = 3; tho[j] = j - 40; }
    }
    for (int i = 0; i < T.np; ++i) {
        if (i < 4) pk[i] = 0;
        else if (i < T.off_beta) { int ip = i - T.off_pose; pk[i] = 1; pa[i] = 3 + ip; pb[i] = ip; }
        else if (i < T.off_orient) pk[i] = 2;
        else if (i < T.off_orient + 3) { pk[i] = 1; pa[i] = i - T.off_orient; }
        else if (i < off_reye) { pk[i] = 1; pa[i] = 23 * 3 + (i - off_leye); }
        else if (i < T.off_lh) { pk[i] = 1; pa[i] = 24 * 3 + (i - off_reye); }
        else if (i < T.off_rh) { pk[i] = 3; pa[i] = 0; pb[i] = i - T.off_lh; }
        else { pk[i] = 3; pa[i] = 1; pb[i] = i - T.off_rh; }
    }
    return r;
}
// loss joints -> chain joint (kind 0) or selector-vertex slot (kind 1) (loss.py:163, models/smpl.py:75); `sel`: the selector
// vertices they read, in order of first use
struct LossJoints { std::vector<int> kind, index, sel; };
LossJoints route_loss_joints(const bf_model_desc *d, int nl) {
    const int nj = d->n_joints;
    LossJoints r;
    for (int k = 0; k < nl; ++k) {
        const int s = d->joint_map[k];
        if (s < nj) { r.kind.push_back(0); r.index.push_back(s); continue; }
        auto it = std::find(r.sel.begin(), r.sel.end(), d->selector_ids[s - nj]);
        if (it == r.sel.end()) { r.sel.push_back(d->selector_ids[s - nj]); it = r.sel.end() - 1; }
        r.kind.push_back(1); r.index.push_back((int)(it - r.sel.begin()));
    }
    return r;
}
// Deal pairs and selector vertices to the four geometry waves (FitTab::pair_slot / skin_vert / bd_ok): pairs with the most selector
// vertices first, each to the wave that already owns its vertices, else to the wave with the fewest vertices, then the fewest pairs.
void deal_pairs(FitTab &T, const LossJoints &lj) {
    const int nl = (int)lj.kind.size(), ns = (int)lj.sel.size(), npairs = (nl + 1) / 2;
    for (int &x : T.pair_slot) x = -1;
    for (int &x : T.skin_vert) x = -1;
    T.bd_ok = (npairs >= 1 && npairs <= 16 && ns <= 4 * BF_SKIN_PER_WAVE) ? 1 : 0;
    std::vector<int> owner(ns, -1), order(std::max(npairs, 0)), nverts(4, 0), npw(4, 0);
    auto verts_of = [&](int p) {
        std::vector<int> v;
        for (int l = 2 * p; l < std::min(2 * p + 2, nl); ++l)
            if (lj.kind[l] == 1 && std::find(v.begin(), v.end(), lj.index[l]) == v.end()) v.push_back(lj.index[l]);
        return v;
    };
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return verts_of(a).size() > verts_of(b).size(); });
    for (int p : order) {
        if (!T.bd_ok) break;
        const std::vector<int> v = verts_of(p);
        int w = -1;
        for (int x : v) if (owner[x] >= 0) { if (w >= 0 && w != owner[x]) T.bd_ok = 0; w = owner[x]; }
        int fresh = 0;
        for (int x : v) if (owner[x] < 0) ++fresh;
        if (w < 0) {
            for (int c = 0; c < 4; ++c) {
                if (npw[c] >= 4 || nverts[c] + fresh > BF_SKIN_PER_WAVE) continue;
                if (w < 0 || nverts[c] < nverts[w] || (nverts[c] == nverts[w] && npw[c] < npw[w])) w = c;
            }
        }
        if (w < 0 || npw[w] >= 4 || nverts[w] + fresh > BF_SKIN_PER_WAVE) { T.bd_ok = 0; break; }
        T.pair_slot[4 * w + npw[w]++] = p;
        for (int x : v) if (owner[x] < 0) { owner[x] = w; T.skin_vert[BF_SKIN_PER_WAVE * w + nverts[w]++] = x; }
    }
    for (int x = 0; x < ns && T.bd_ok; ++x) if (owner[x] < 0) T.bd_ok = 0;       // (a selector vertex no pair reads: cannot happen, sel is built from the loss joints)
}

// ---- sub-models (bf_model::Sub): the model's tables gathered for a subset of its vertices --------------------------------------
//   sub     "sampled first": every 4th vertex (the silhouette loss, loss.py:99) first, then what the dense keypoint loss reads;
//   sub_kp  (round 5) only what the dense keypoint loss reads - selector vertices, the landmark faces' corners, the support of
//           the extra regressor: the iterations BEFORE the silhouette / scan losses switch on (i <= num_iters // 3,
//           smplify.py:197,205) touch nothing else, with or without a scan attached.
struct SubTables { bool on = false; int n_samp = 0, nv = 0; std::vector<int> selector_ids, faces, verts; Gather g; Corners lmk; };
// off (the full model serves) when it would hold more than max_tenths / 10 of the vertices; `kv` flags the vertices the dense
// keypoint loss reads, `nnz` is the full model's sparse skinning width
SubTables derive_sub(const bf_model_desc *d, const std::vector<char> &kv, bool sampled_first, int max_tenths, int nnz) {
    const int nv = d->n_verts;
    std::vector<int> pos(nv, -1), verts;
    if (sampled_first) for (int v = 0; v < nv; v += 4) { pos[v] = (int)verts.size(); verts.push_back(v); }
    SubTables s;
    s.n_samp = (int)verts.size();
    for (int v = 0; v < nv; ++v) if (kv[v] && pos[v] < 0) { pos[v] = (int)verts.size(); verts.push_back(v); }
    s.nv = (int)verts.size();
    if (s.nv == 0 || s.nv * 10 > nv * max_tenths) return SubTables{};
    s.on = true;
    s.verts = verts;
    s.g = gather_vertices(d, verts, pd_pitch_of(3 * s.nv), nnz);
    for (int i = 0; i < d->n_selector; ++i) s.selector_ids.push_back(pos[d->selector_ids[i]]);
    if (d->model_kind == 1) {            // faces re-indexed; a corner outside the sub-model belongs to a face no landmark uses
        for (int i = 0; i < d->n_faces * 3; ++i) s.faces.push_back(std::max(pos[d->faces[i]], 0));
        s.lmk = landmark_corners(d, s.faces.data());
    }
    return s;
}
struct HostTables {
    FitTab fit;                       // scalar fields and the pair deal (the pointers are filled on upload)
    Tree tree; LossJoints lj; Regressor reg;
    Gather full, sel;                 // all vertices in order, pitch padded; the selector vertices, pitch 3 ns, BF_SEL_NNZ wide
    int v_nnz = 0;                    // MeshTab::v_nnz: 4 or 8, 0 when some vertex has more than 8 bones
    GmmImages gmm; Routing route; Corners lmk;
    std::vector<int> kp_jm, cj_start, cj_list;     // dense keypoint loss: loss joint -> all-joints index; per chain joint its loss joints
    SubTables sub, sub_kp;
};
HostTables derive_tables(const bf_model_desc *d) {
    const int nv = d->n_verts, nj = d->n_joints;
    const bool kp_dense = d->n_loss_joints > 32;
    HostTables H;
    H.tree = derive_tree(d);
    H.lj = route_loss_joints(d, kp_dense ? 0 : d->n_loss_joints);
    H.fit = fit_sizes(d, (int)H.lj.kind.size(), (int)H.lj.sel.size(), H.tree.n_levels);
    deal_pairs(H.fit, H.lj);
    H.route = route_params(H.fit);
    H.reg = contract_regressor(d);
    H.sel = gather_vertices(d, H.lj.sel, 3 * (int)H.lj.sel.size(), BF_SEL_NNZ);
    H.fit.sel_nnz = H.sel.max_nnz <= BF_SEL_NNZ ? H.sel.max_nnz : 0;
    std::vector<int> all(nv);
    std::iota(all.begin(), all.end(), 0);
    int most = 0;                         // the most bones of one vertex
    for (const float *w = d->lbs_weights; w < d->lbs_weights + (size_t)nv * nj; w += nj) most = std::max(most, nj - (int)std::count(w, w + nj, 0.f));
    H.v_nnz = most <= 4 ? 4 : (most <= 8 ? 8 : 0);
    H.full = gather_vertices(d, all, pd_pitch_of(3 * nv), H.v_nnz);
    H.gmm = gmm_images(d);
    if (d->model_kind == 1) H.lmk = landmark_corners(d, d->faces);
    if (kp_dense) {
        H.kp_jm.assign(d->joint_map, d->joint_map + d->n_loss_joints);
        for (int j = 0; j < nj; ++j) {
            H.cj_start.push_back((int)H.cj_list.size());
            for (int q = 0; q < d->n_loss_joints; ++q) if (H.kp_jm[q] == j) H.cj_list.push_back(q);
        }
        H.cj_start.push_back((int)H.cj_list.size());
        if (H.cj_list.empty()) H.cj_list.push_back(0);
    }
    std::vector<char> kv(nv, 0);          // the vertices the dense keypoint loss reads
    for (int i = 0; i < d->n_selector; ++i) kv[d->selector_ids[i]] = 1;
    for (int i = 0; d->model_kind == 1 && i < d->n_lmk_static * 3; ++i) kv[H.lmk.sfv[i]] = 1;
    for (size_t i = 0; d->model_kind == 1 && i < n_dyn(d) * 3; ++i) kv[H.lmk.dfv[i]] = 1;
    // (the extra-joint regressor rows are gathered for the sub-model's vertices: every vertex that carries regressor weight
    //  must be one of them, or the extra joints of the dense loop would be partial sums)
    for (int e = 0; e < d->n_extra; ++e)
        for (int v = 0; v < nv; ++v) if (d->j_regressor_extra[(size_t)e * nv + v] != 0.f) kv[v] = 1;
    H.sub = derive_sub(d, kv, true, 6, H.v_nnz);
    if (kp_dense) H.sub_kp = derive_sub(d, kv, false, 5, H.v_nnz);      // (only models whose keypoint loss is dense have keypoint-only dense iterations)
    return H;
}

// ---- upload: each table struct uploads what it points at and takes the pointers ------------------------------------------------

// uploads until the first failure, which it keeps; -> the device copy (null after a failure)
struct Uploader {
    hipError_t err = hipSuccess;
    template <class T> T *operator()(DevBuf<T> &b, const std::vector<T> &h) { if (err == hipSuccess) err = b.upload(h); return b.p; }
    template <class T> T *operator()(DevBuf<T> &b, const T *src, size_t n) { return (*this)(b, std::vector<T>(src, src + n)); }
};

void fill_fit(Uploader &up, bf_model &m, const bf_model_desc *d, const HostTables &H) {
    FitTab &T = m.fit = H.fit;
    const Tree &t = H.tree;
    T.parents = up(m.parents, d->parents, (size_t)m.nj); T.depth = up(m.depth_d, t.depth); T.desc = up(m.desc_d, t.desc);
    T.dfs_order = up(m.dfs_order, t.dfs_order); T.dfs_last = up(m.dfs_last, t.dfs_last);
    T.level_start = up(m.level_start, t.level_start); T.level_joints = up(m.level_joints, t.level_joints);
    T.child_start = up(m.child_start, t.child_start); T.child_list = up(m.child_list, t.child_list);
    T.lj_kind = up(m.lj_kind, H.lj.kind); T.lj_index = up(m.lj_index, H.lj.index);
    T.th_kind = up(m.th_kind, H.route.th_kind); T.th_off = up(m.th_off, H.route.th_off);
    T.p_kind = up(m.p_kind, H.route.p_kind); T.p_a = up(m.p_a, H.route.p_a); T.p_b = up(m.p_b, H.route.p_b);
    T.Jt = up(m.Jt, H.reg.Jt); T.Jd = up(m.Jd, H.reg.Jd); T.Jdrel = up(m.Jdrel, H.reg.Jdrel); T.Jtrel = up(m.Jtrel, H.reg.Jtrel);
    T.sel_vt = up(m.sel_vt, H.sel.vt); T.sel_sd = up(m.sel_sd, H.sel.sd); T.sel_pd = up(m.sel_pd, H.sel.pd); T.sel_w = up(m.sel_w, H.sel.lw);
    T.sel_nzw = up(m.sel_nzw, H.sel.zw); T.sel_nzj = up(m.sel_nzj, H.sel.zj);
    T.g_means = up(m.g_means, H.gmm.means); T.g_psym = up(m.g_psym, H.gmm.psym); T.g_logw = up(m.g_logw, H.gmm.logw);
    T.g_plane = up(m.g_plane, H.gmm.plane); T.g_ptail = up(m.g_ptail, H.gmm.ptail);
    if (d->model_kind == 1) {               // the full pose's SMPL-X terms (null for SMPL)
        const size_t n_comp = (size_t)d->n_hand_pca * 45;
        std::vector<float> hc(d->left_hand_components, d->left_hand_components + n_comp);
        hc.insert(hc.end(), d->right_hand_components, d->right_hand_components + n_comp);
        T.hand_comp = up(m.hand_comp, hc); T.pose_mean = up(m.pose_mean, d->pose_mean, (size_t)d->n_joints * 3);
    }
}
void fill_mesh(Uploader &up, bf_model &m, const bf_model_desc *d, const HostTables &H) {
    MeshTab &Q = m.mesh;
    Q.nv = m.nv; Q.nj = m.nj; Q.nb = m.nb; Q.npf = m.npf;
    Q.n_selector = d->n_selector; Q.n_extra = d->n_extra; Q.n_joint_map = d->n_joint_map;
    Q.n_tiles = (m.nv + BF_MESH_TILE - 1) / BF_MESH_TILE; Q.pd_pitch = pd_pitch_of(3 * m.nv); Q.v_nnz = H.v_nnz;
    Q.v_template = up(m.v_template, H.full.vt); Q.shapedirs = up(m.shapedirs, H.full.sd); Q.posedirs = up(m.posedirs, H.full.pd);
    Q.lbs_weights = up(m.lbs_weights, H.full.lw); Q.j_extra = up(m.j_extra, H.full.jx);
    Q.v_nzj = up(m.v_nzj, H.full.zj); Q.v_nzw = up(m.v_nzw, H.full.zw);
    Q.selector_ids = up(m.selector_ids, d->selector_ids, d->n_selector); Q.joint_map = up(m.joint_map, d->joint_map, d->n_joint_map);
    if (d->model_kind != 1) return;
    Q.n_lmk_static = d->n_lmk_static; Q.n_lmk_dyn = d->n_lmk_dynamic; Q.n_dyn_rows = d->n_dyn_rows; Q.neck_joint = d->neck_joint;
    Q.faces = up(m.faces_lm, d->faces, (size_t)d->n_faces * 3);
    Q.lmk_faces = up(m.lmk_faces, d->lmk_faces_idx, d->n_lmk_static); Q.lmk_bary = up(m.lmk_bary, d->lmk_bary_coords, (size_t)d->n_lmk_static * 3);
    Q.dyn_faces = up(m.dyn_faces, d->dynamic_lmk_faces_idx, n_dyn(d)); Q.dyn_bary = up(m.dyn_bary, d->dynamic_lmk_bary_coords, n_dyn(d) * 3);
    Q.lmk_fv = up(m.lmk_fv, H.lmk.sfv); Q.dyn_fv = up(m.dyn_fv, H.lmk.dfv);
}
void fill_kp(Uploader &up, bf_model &m, const bf_model_desc *d, const HostTables &H) {
    if (!m.kp_dense) return;
    KpIO &K = m.kp;
    K.nl = m.nl_loss; K.nj = m.nj; K.npf = m.npf; K.nb = m.nb; K.nv = m.nv; K.n_all = m.n_all; K.n_selector = d->n_selector;
    K.n_extra = d->n_extra; K.n_lmk = m.n_lmk; K.n_cj_list = (int)H.cj_list.size();
    K.joint_map = up(m.kp_jm, H.kp_jm); K.cj_start = up(m.cj_start, H.cj_start); K.cj_list = up(m.cj_list, H.cj_list);
    K.selector_ids = m.selector_ids.p; K.j_extra = m.j_extra.p;
}
// the full model's MeshTab / KpIO over the sub-model's vertices
void fill_sub(Uploader &up, bf_model::Sub &U, const bf_model &m, const SubTables &s) {
    if (!s.on) return;
    MeshTab &Q = U.mesh = m.mesh;
    Q.nv = s.nv; Q.n_tiles = (s.nv + BF_MESH_TILE - 1) / BF_MESH_TILE; Q.pd_pitch = pd_pitch_of(3 * s.nv);
    Q.v_template = up(U.v_template, s.g.vt); Q.shapedirs = up(U.shapedirs, s.g.sd); Q.posedirs = up(U.posedirs, s.g.pd);
    Q.lbs_weights = up(U.lbs_weights, s.g.lw); Q.j_extra = up(U.j_extra, s.g.jx);
    Q.v_nzj = up(U.v_nzj, s.g.zj); Q.v_nzw = up(U.v_nzw, s.g.zw); Q.selector_ids = up(U.selector_ids, s.selector_ids);
    if (!s.faces.empty()) { Q.faces = up(U.faces, s.faces); Q.lmk_fv = up(U.lmk_fv, s.lmk.sfv); Q.dyn_fv = up(U.dyn_fv, s.lmk.dfv); }
    U.kp = m.kp; U.kp.nv = s.nv; U.kp.selector_ids = Q.selector_ids; U.kp.j_extra = Q.j_extra;
    up(U.verts, s.verts); U.verts_host = s.verts;
    U.ns = s.n_samp; U.on = true;
}

}  // namespace

extern "C" {

int bf_model_create(const bf_model_desc *d, int device, bf_model **out) {
    if (!d || !out) return fail(BF_ERR_INVALID, "bf_model_create: null argument");
    *out = nullptr;
    if (bf_device_count() <= device || device < 0) return fail(BF_ERR_NO_DEVICE, "bf_model_create: no such HIP device");
    if (int rc = check_desc(d)) return rc;
    HIP_TRY(hipSetDevice(device));

    const HostTables H = derive_tables(d);
    std::unique_ptr<bf_model> m(new bf_model());
    m->device = device;
    m->nv = d->n_verts; m->nj = d->n_joints; m->nb = d->n_betas; m->npf = H.fit.npf;
    m->n_selector = d->n_selector; m->n_extra = d->n_extra; m->n_joint_map = d->n_joint_map;
    m->ns = H.fit.ns; m->nl = H.fit.nl; m->np = H.fit.np; m->n_levels = H.fit.n_levels;
    m->kind = d->model_kind; m->n_all = n_all_joints(d); m->n_lmk = d->model_kind == 1 ? d->n_lmk_static + d->n_lmk_dynamic : 0;
    m->kp_dense = H.fit.kp_dense; m->nl_loss = d->n_loss_joints;     // (kp_dense: the keypoint loss goes through bf_kp_loss_kernel, nl = 0)
    m->mesh_smem = bf_mesh_smem_bytes(m->nj, m->npf, m->nb);
    if (d->n_faces > 0 && d->faces) m->faces_host.assign(d->faces, d->faces + (size_t)d->n_faces * 3);
    if (m->kind == 1) {                   // the joint regressor's non-zeros stay on the host: bf_model_set_expression contracts it with E
        for (int j = 0; j < m->nj; ++j) {
            m->jreg_start.push_back((int)m->jreg_v.size());
            for (int v = 0; v < m->nv; ++v)
                if (const float w = d->j_regressor[(size_t)j * m->nv + v]; w != 0.f) { m->jreg_v.push_back(v); m->jreg_w.push_back(w); }
        }
        m->jreg_start.push_back((int)m->jreg_v.size());
    }

    Uploader up;
    fill_fit(up, *m, d, H);
    fill_mesh(up, *m, d, H);
    fill_kp(up, *m, d, H);
    fill_sub(up, m->sub, *m, H.sub);
    fill_sub(up, m->sub_kp, *m, H.sub_kp);
    if (up.err != hipSuccess) return fail(BF_ERR_HIP, std::string("bf_model_create: device allocation / upload failed: ") + hipGetErrorString(up.err));
    *out = m.release();
    return BF_OK;
}

void bf_model_destroy(bf_model *model_handle) { std::unique_ptr<bf_model> drop(model_handle); }
int bf_model_n_params(const bf_model *m) { return m ? m->np : 0; }
int bf_model_sub_vertices(const bf_model *m, int which, int32_t *ids) {
    if (!m || which < 0 || which > 1) return fail(BF_ERR_INVALID, "bf_model_sub_vertices: bad argument");
    const bf_model::Sub &U = which ? m->sub_kp : m->sub;
    if (!U.on) return 0;
    if (ids) std::copy(U.verts_host.begin(), U.verts_host.end(), ids);
    return (int)U.verts_host.size();
}
int bf_model_fit_instance(const bf_model *m) { return (m && bf_fit_is_sized_smpl(&m->fit)) ? 1 : 0; }

// generic forward from packed parameters (bf_model_forward): a stateless call on host arrays, on the host route of a BfRouteCall
int bf_model_forward(bf_model *m, int n, const float *params, float *vertices, float *joints) {
    if (!m || n <= 0 || !params) return fail(BF_ERR_INVALID, "bf_model_forward: bad argument");
    BfRouteCall c(nullptr, nullptr);
    BF_TRY(c.begin(m->device));
    const size_t N = (size_t)n;
    // model space: similarity parameters are ignored (transl 0, scale 1, constant scale 1)
    std::vector<float> pk(params, params + N * m->np);
    for (int i = 0; i < n; ++i) { float *q = pk.data() + (size_t)i * m->np; q[0] = q[1] = q[2] = 0.f; q[3] = 1.f; }
    const float *d_p = nullptr;
    float *d_state = nullptr, *d_vraw = nullptr, *d_j = nullptr, *d_xp = nullptr;
    BF_TRY(c.in(pk.data(), pk.size(), d_p));
    BF_TRY(c.scratch(N * bf_state_stride(m->nj, m->npf, m->nb), d_state));
    BF_TRY(c.out(vertices, N * m->nv * 3, d_vraw, true));
    BF_TRY(c.out(joints, N * m->n_joint_map * 3, d_j, true));
    BF_TRY(c.scratch(N * m->mesh.n_tiles * std::max(m->n_extra, 1) * 3, d_xp));
    hipLaunchKernelGGL(bf_pose_state_kernel, dim3(n), dim3(128), 0, c.stream, m->fit, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, d_state, d_p, (const float *)nullptr, 1.0f);
    HIP_TRY(hipGetLastError());
    MeshPass mesh;
    mesh.scr = c.mesh_scratch(); mesh.n = n; mesh.state = d_state; mesh.stream = c.stream;
    mesh.vraw = d_vraw; mesh.xpart = d_xp; mesh.joints = d_j;
    BF_TRY(bf_launch_mesh(m, mesh));
    return c.finish();
}

}  // extern "C"
