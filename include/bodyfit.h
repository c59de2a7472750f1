/*
 * libbodyfit - MI355X-native multi-view SMPLify inner loop, C ABI.
 *
 * The reference (generalizable-neural-performer/bodyfitting) has no C/plugin API for this path;
 * its boundary is Python (`smplify.smplify.SMPLify`, `smplify.body_fitting.BodyFitting`,
 * `models.smpl.SMPL`).  This header is the native surface the build's Python mirror of those
 * classes (bodyfitting_amd/smplify.py, smpl.py) binds through ctypes.  Each entry point names the
 * reference code it replaces.
 *
 * Conventions: every function returns 0 on success and a negative bf_status otherwise;
 * bf_last_error() gives the message for the calling thread.  All pointers are HOST pointers to
 * caller-owned, C-contiguous buffers unless the name ends in `_dev`.  Device memory is owned by the
 * library behind the opaque handles.  One handle is used by one host thread at a time.  Work is
 * queued on the batch's own HIP stream; nothing blocks except bf_batch_sync and the getters.
 * All floating point is fp32 (the reference's dtype); indices are int32.
 */
#ifndef BODYFIT_H
#define BODYFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden visibility: what is declared in here, and nothing else, is exported */
#pragma GCC visibility push(default)

typedef enum bf_status {
    BF_OK = 0,
    BF_ERR_INVALID = -1,      /* bad argument / inconsistent sizes */
    BF_ERR_HIP = -2,          /* a HIP runtime call failed (message has the hipError string) */
    BF_ERR_UNSUPPORTED = -3,  /* size outside what the kernels were built for */
    BF_ERR_NO_DEVICE = -4     /* no usable gfx950 device */
} bf_status;

typedef struct bf_model bf_model;   /* body model + GMM prior resident on one device */
typedef struct bf_batch bf_batch;   /* F independent frames being fitted against one model */
typedef struct bf_scan bf_scan;     /* one scan mesh + its uniform closest-point grid on one device */

/*
 * Body model tensors exactly as smplx==0.1.13 stores them and reference models/smpl.py:56-66 extends
 * them, plus the buffers of MaxMixturePrior (reference smplify/prior.py:143-160).
 */
typedef struct bf_model_desc {
    int32_t n_verts;               /* NV: 6890 (SMPL) */
    int32_t n_joints;              /* NJ: 24 */
    int32_t n_betas;               /* NB: 10 */
    const float *v_template;       /* [NV,3] */
    const float *shapedirs;        /* [NV,3,NB] */
    const float *posedirs;         /* [9(NJ-1), 3NV]  row p = pose-feature element, col = 3v+k */
    const float *j_regressor;      /* [NJ,NV] dense */
    const float *lbs_weights;      /* [NV,NJ] dense */
    const int32_t *parents;        /* [NJ], parents[0] = -1, parents[i] < i */
    int32_t n_selector;            /* 21: VertexJointSelector vertex ids appended after the chain joints */
    const int32_t *selector_ids;   /* [n_selector] */
    int32_t n_extra;               /* 9: rows of J_regressor_extra (models/smpl.py:62-64,72) */
    const float *j_regressor_extra;/* [n_extra,NV] dense */
    int32_t n_joint_map;           /* 49: output joints = cat(chain, selector, extra)[joint_map] */
    const int32_t *joint_map;      /* [n_joint_map] (models/smpl.py:61,75) */
    int32_t n_loss_joints;         /* 25: SKELETON_LENGTH, the leading joints that enter the loss (loss.py:17,163) */
    int32_t gmm_components;        /* 8 */
    int32_t gmm_dim;               /* 69 */
    const float *gmm_means;        /* [M,D] */
    const float *gmm_precisions;   /* [M,D,D] = inv(covars) */
    const float *gmm_nll_weights;  /* [M] (prior.py:153-160) */
    int32_t n_faces;               /* body-model topology, only needed by the SMPL+D stage; may be 0 */
    const int32_t *faces;          /* [n_faces,3] */
    /* ---- SMPL-X (smplx.create(model_type='smplx', use_face_contour=True, use_pca with 6 comps), smplify.py:59-80).
     * model_kind 0 = SMPL (everything below ignored), 1 = SMPL-X: joints 0 root, 1..21 body, 22 jaw, 23/24 eyes,
     * 25..39 / 40..54 left / right hand; n_betas = 10 (the expression directions are attached apart, by bf_model_set_expression;
     * the fit leaves expression at 0, smplify.py:167-173); the optimised
     * vector is transl3 scale1 body_pose63 betas10 global_orient3 leye3 reye3 left_hand_pca6 right_hand_pca6 (98). */
    int32_t model_kind;
    const float *pose_mean;                 /* [3 NJ], added to the assembled full pose */
    int32_t n_hand_pca;                     /* 6 */
    const float *left_hand_components;      /* [n_hand_pca,45] */
    const float *right_hand_components;     /* [n_hand_pca,45] */
    int32_t n_lmk_static;                   /* 51 */
    const int32_t *lmk_faces_idx;           /* [n_lmk_static] face ids */
    const float *lmk_bary_coords;           /* [n_lmk_static,3] */
    int32_t n_lmk_dynamic;                  /* 17 */
    int32_t n_dyn_rows;                     /* 79 */
    const int32_t *dynamic_lmk_faces_idx;   /* [n_dyn_rows,n_lmk_dynamic] */
    const float *dynamic_lmk_bary_coords;   /* [n_dyn_rows,n_lmk_dynamic,3] */
    int32_t neck_joint;                     /* 12: its global rotation's yaw picks the contour row */
} bf_model_desc;

/* Loss weights and optimiser constants; bf_hyper_default() fills the reference's literals. */
typedef struct bf_hyper {
    float sigma;               /* 100   loss.py:139 */
    float pose_prior_weight;   /* 4.78  loss.py:141 */
    float angle_prior_weight;  /* 15.2  loss.py:140 */
    float shape_prior_weight;  /* 5     loss.py:140 */
    float constant_scale;      /* 0.3   smplify.py:160 */
    float imsize;              /* 512   scale_coeff = imsize/1024, loss.py:155 */
    float lr;                  /* 1e-2  smplify.py:174 */
    float lr_transl_scale;     /* 0.1   smplify.py:167-168 */
    float adam_beta1;          /* 0.9 */
    float adam_beta2;          /* 0.999 */
    float adam_eps;            /* 1e-8 */
    float lr_displacement;     /* 5e-2  smplify.py:233 */
    float mask_cdist_form;     /* 1     silhouette loss: 1 = contour-to-vertex distances in the fp32 form torch.cdist evaluates for
                                        these sizes (loss.py:108: |a|^2 + |b|^2 - 2ab as one 4-term fma chain, ~1e-2 px of
                                        round-off at 512 px - the reference's own numbers, so the nearest-vertex choice matches
                                        it); 0 = exact (a - b)^2 sums */
    float dense_after;         /* -1    the silhouette / scan losses are active for iterations i > dense_after, i counted from the
                                        last reset; -1 = num_iters // 3 of the bf_fit call (smplify.py:197,205).  Lets a caller
                                        cut one reference loop into several bf_fit calls (snapshots) */
} bf_hyper;

/* bf_fit flags */
#define BF_FIT_DEFAULT      0u
#define BF_FIT_DENSE        1u   /* evaluate the full mesh every iteration, like the reference does
                                    (smplify.py:179-190), instead of only the vertices that carry
                                    gradient; same results, used for measurement */
#define BF_FIT_NO_VERTICES  2u   /* skip the final full-mesh evaluation (parameters only) */
#define BF_FIT_RESET        8u   /* bf_batch_reset() first, inside the same call */
#define BF_FIT_GRAPH       16u   /* with BF_FIT_RESET on the keypoint-only path: capture the call's whole command sequence
                                    into a hipGraph once and replay it - one host command per fit (per-kernel device times are
                                    then not split: bf_batch_last_timing charges everything to ms[0]) */
#define BF_FIT_NOTIME      32u   /* do not bracket the parts of this call with HIP events (bf_batch_last_timing / timing_sum skip it):
                                     four event records per call are a measurable share of a 0.65 ms step.  With BF_FIT_RESET |
                                     BF_FIT_FETCH on the keypoint-only path the mesh / joints / result hand-over of the call then runs
                                     on the batch's second stream, under the fit kernel of the NEXT call (frame after frame) */
#define BF_FIT_FETCH        4u   /* queue the device->host copies of the result into the batch's pinned
                                    staging buffers behind the kernels (bf_batch_get_result then only
                                    waits for them) */

const char *bf_last_error(void);
const char *bf_version(void);
int bf_device_count(void);
void bf_hyper_default(bf_hyper *h);

/* Replaces the per-frame model + prior construction of SMPLify.__init__ (smplify.py:46-56): the
 * tensors are uploaded once per process, and the model-level tables of the fit are derived. */
int bf_model_create(const bf_model_desc *desc, int device, bf_model **out);
void bf_model_destroy(bf_model *m);
/* number of optimised scalars per frame: 86 for SMPL, laid out in the reference's optimiser order
 * (smplify.py:167-171): global_transl[3] body_scale[1] body_pose[69] betas[10] global_orient[3] */
int bf_model_n_params(const bf_model *m);
/* which instance of the persistent keypoint fit this model takes (no reference counterpart: the reference has one code path):
 * 1 = sizes fixed at compile time (24 joints, 10 betas, 11 loss selector vertices with at most 4 bones each, 25 loss joints: SMPL
 * as models/smpl.py:56-66 builds it), 0 = table-driven (any other model; ~2.5x more cycles per iteration) */
int bf_model_fit_instance(const bf_model *m);
/* test hook: the full-model vertex ids of a sub-model the dense iterations run on, in the sub-model's order.  which = 0: the
 * "sampled first" sub-model (every 4th vertex, then what the keypoint loss reads), 1: the keypoint-only one.  -> their number
 * (0: the model has no such sub-model); ids may be NULL. */
int bf_model_sub_vertices(const bf_model *m, int which, int32_t *ids);


/* models.smpl.SMPL.forward (models/smpl.py:69-83) for `n` parameter sets:
 * betas[n,NB], global_orient[n,3], body_pose[n,3(NJ-1)] ->
 * vertices[n,NV,3], joints[n,n_joint_map,3], joints_ori[n,NJ+n_selector,3] (either output may be NULL) */
int bf_smpl_forward(bf_model *m, int n, const float *betas, const float *global_orient,
                    const float *body_pose, float *vertices, float *joints, float *joints_ori);

/* models.smpl.SMPL.forward's vector-Jacobian product: the backward torch.autograd runs through smplx's lbs() and the
 * wrapper of models/smpl.py:69-83, for `n` parameter sets betas[n,NB], global_orient[n,3], body_pose[n,3(NJ-1)].
 * Cotangents dvertices[n,NV,3], djoints[n,n_joint_map,3], djoints_ori[n,NJ+n_selector,3] (any may be NULL = zero) ->
 * dbetas[n,NB], dglobal_orient[n,3], dbody_pose[n,3(NJ-1)] (any may be NULL = not wanted).  SMPL-kind models only
 * (SMPL-X: BF_ERR_UNSUPPORTED).  Stateless: the pose state and the pose-blended vertices are recomputed by the call; every
 * sum has a fixed order, so equal inputs give equal bits. */
int bf_smpl_vjp(bf_model *m, int n, const float *betas, const float *global_orient, const float *body_pose,
                const float *dvertices, const float *djoints, const float *djoints_ori,
                float *dbetas, float *dglobal_orient, float *dbody_pose);

/* smplx.create(model_type='smplx', use_pca=True, flat_hand_mean=False, use_face_contour=True)'s forward (smplify.py:59-80,
 * 177-190) and its vector-Jacobian product for `n` parameter sets of an SMPL-X-kind model; SMPL-kind models: BF_ERR_UNSUPPORTED.
 * `expression` is an input of the _expr variants below, on a model bf_model_set_expression gave its directions to; the device
 * model itself carries the shape directions only (bf_model_create: n_betas <= 12), and the fit never optimises expression
 * (smplify.py:167-173). */
typedef struct bf_smplx_params {          /* betas, global_orient, body_pose are required; a NULL among the others = zeros */
    const float *betas;                    /* [n,NB]; [n,n_betas] after bf_model_set_shape_space (bf_model_n_betas) */
    const float *global_orient;            /* [n,3] */
    const float *body_pose;                /* [n,63] */
    const float *jaw_pose, *leye_pose, *reye_pose;           /* [n,3] each */
    const float *left_hand_pose, *right_hand_pose;           /* [n,n_hand_pca] PCA coefficients */
} bf_smplx_params;
typedef struct bf_smplx_outputs {         /* model space, no similarity; any may be NULL */
    float *vertices;                       /* [n,NV,3] */
    float *joints;                         /* [n,n_joint_map,3]: the 135 joints of the model's joint_map */
    float *joints_all;                     /* [n,NJ+n_selector+n_extra+68,3]: the 144 joints smplx returns before a joint_mapper */
    float *full_pose;                      /* [n,3 NJ]: the assembled pose, pose_mean included */
    int32_t *dyn_row;                      /* [n]: the row of the contour table the neck chain's yaw selects */
} bf_smplx_outputs;
typedef struct bf_smplx_cotangents {      /* shapes of bf_smplx_outputs; a NULL = zero */
    const float *dvertices, *djoints, *djoints_all, *dfull_pose;
} bf_smplx_cotangents;
typedef struct bf_smplx_grads {           /* shapes of bf_smplx_params; a NULL = not wanted */
    float *dbetas, *dglobal_orient, *dbody_pose, *djaw_pose, *dleye_pose, *dreye_pose, *dleft_hand_pose, *dright_hand_pose;
} bf_smplx_grads;
/* With jaw_pose NULL, `vertices` and `joints` are bit for bit bf_model_forward's of the same values in packed order. */
int bf_smplx_forward(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_outputs *out);
/* Stateless like bf_smpl_vjp: the forward is recomputed by the call; every sum has a fixed order (no float atomics), so equal
 * inputs give equal bits.  The contour landmarks' row is an integer look-up: no gradient flows through the choice, only through
 * the barycentric combination of the chosen faces' vertices. */
int bf_smplx_vjp(bf_model *m, int n, const bf_smplx_params *in, const bf_smplx_cotangents *cot, const bf_smplx_grads *grads);

/* SMPL-X expression coefficients (smplx lbs(): v_shaped = v_template + shapedirs betas + exprdirs expression, the rest joints
 * regressed from it).  bf_model_set_expression attaches exprdirs[NV,3,n_expr] - the columns behind the 10 shape directions of an
 * SMPL-X file's shapedirs - to an SMPL-X-kind model, once, before any call that uses them: SMPL-kind models and n_expr outside
 * 1..16 are BF_ERR_UNSUPPORTED, a second call is BF_ERR_INVALID.
 * bf_model_n_expression: their number, 0 when none is attached. */
int bf_model_set_expression(bf_model *m, int n_expr, const float *exprdirs);
int bf_model_n_expression(const bf_model *m);
/* A wider shape space for the four smplx entry points below and their _dev twins: n_betas (10..300) is the number of betas they
 * then take, n_expr (0..100) the number of expression coefficients, and dirs[NV,3,(n_betas-10)+n_expr] holds the shape directions
 * from the eleventh on followed by the expression directions (an SMPL-X v1.1 file: columns 10:n_betas and 300:300+n_expr).  At
 * least one direction; values outside those ranges and SMPL-kind models are BF_ERR_UNSUPPORTED.  Attached once, instead of
 * bf_model_set_expression: after either call the other one, or the same one again, is BF_ERR_INVALID.  Afterwards betas is
 * [n,n_betas], dbetas [n,n_betas], expression [n,n_expr] (NULL = zero coefficients; dexpression must then be NULL) and
 * dexpression [n,n_expr].  The ten core betas stay where they are - in the device model, the fit and bf_model_forward, which know
 * nothing of the rest; a frame's other coefficients [betas[10:], expression] go around the model's passes the way expression
 * does.  Up to 16 such directions run on the kernels behind bf_model_set_expression, more on kernels of their own that walk the
 * directions once per block of 8 frames (the environment variable BF_SHAPE_EXT_WIDE=1, read at either attachment, sends any
 * number through those); both keep every sum in a fixed order.  Device memory: the directions once, and a second time in
 * [NV,3,L] order for the wide reverse - 2 x 12 NV L bytes.
 * bf_model_n_betas: the betas a call takes - n_betas after the attachment, else the model's own.
 * bf_model_shape_ext_wide: 1 when the attached directions run on the wide kernels, else 0. */
int bf_model_set_shape_space(bf_model *m, int n_betas, int n_expr, const float *dirs);
int bf_model_n_betas(const bf_model *m);
int bf_model_shape_ext_wide(const bf_model *m);
/* bf_smplx_forward / bf_smplx_vjp with expression[n,n_expr]; dexpression[n,n_expr] (NULL = not wanted).  expression == NULL is
 * exactly the call without it: the same launches, the same bits (dexpression must then be NULL).  With expression on a model
 * without directions: BF_ERR_UNSUPPORTED.  Around the unchanged passes of the model, kernels of their own add the expression
 * term, which is affine for fixed rotations; every sum has a fixed order, and a dexpression left NULL changes no other bit.
 * The fit (bf_fit, bf_group_*) and bf_model_forward's packed vector do not take expression. */
int bf_smplx_forward_expr(bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_outputs *out);
int bf_smplx_vjp_expr(bf_model *m, int n, const bf_smplx_params *in, const float *expression, const bf_smplx_cotangents *cot,
                      const bf_smplx_grads *grads, float *dexpression);

/* MaxMixturePrior's buffers (smplify/prior.py:142-160) on one device, uploaded once: means[M,D], precisions[M,D,D],
 * nll_weights[M] (positive).  At most 16 components of at most 128 dimensions (BF_ERR_UNSUPPORTED beyond). */
typedef struct bf_gmm bf_gmm;
int bf_gmm_create(int device, int n_components, int dim, const float *means, const float *precisions,
                  const float *nll_weights, bf_gmm **out);
void bf_gmm_destroy(bf_gmm *g);

/* multiview_keypoint_loss (smplify/loss.py:139-230) for `n` independent problems - each one set of world-space joints, V views,
 * one body pose and one betas vector - and its vector-Jacobian product with respect to joints, poses and betas. */
typedef struct bf_keypoint_loss_in {
    int32_t n, n_views, n_rows;     /* problems, views per problem, joint rows (25 for SMPL, 135 for SMPL-X with hands + face; <= 256) */
    const float *joints;            /* [n,n_rows,3] world space, as smplify.py:189 scales them */
    const float *w2c;               /* [n,V,4,4]; rows 0..2 are read */
    const float *K;                 /* [n,V,3,3] */
    const float *keypoints;         /* [n,V,n_rows,3] x, y, confidence; a group absent from a present view = zero confidences */
    const uint8_t *present;         /* [n,V], NULL = all present; an absent view is skipped, not projected */
    const int32_t *divisor;         /* [n] = len(use_frames), positive */
    int32_t pose_dim;  const float *poses;    /* [n,pose_dim], NULL = no pose / angle prior; pose_dim > 55 and <= the GMM's dim
                                                 (the pose is zero-padded to it, loss.py:206-207) */
    int32_t n_betas;   const float *betas;    /* [n,n_betas], NULL = no shape prior; n_betas <= 16 */
} bf_keypoint_loss_in;
/* terms[n,4] = reprojection, pose prior, angle prior, shape prior (loss.py:219-224), weighted as the reference weights them
 * with sigma, the three prior weights and imsize of `hyper` (NULL: bf_hyper_default; its other fields are not read).
 * djoints[n,n_rows,3], dposes[n,pose_dim], dbetas[n,n_betas] = the gradient of sum(dterms * terms), dterms[n,4] (NULL = ones).
 * `terms` and every gradient may be NULL = not wanted.  gmm NULL: the pose prior term is 0.  The GMM term is the minimum over
 * the components (ties: the lowest), its gradient that of the arg-min component alone.  V = 0 or every view absent: the
 * reprojection term is 0 and djoints exactly 0.  Host pointers; stateless apart from `gmm`; every sum has a fixed order (no
 * float atomics), so equal inputs give equal bits and a problem's result does not depend on its neighbours in the call. */
int bf_keypoint_loss(int device, const bf_gmm *gmm, const bf_keypoint_loss_in *in, const bf_hyper *hyper,
                     const float *dterms, float *terms, float *djoints, float *dposes, float *dbetas);

/* The device route: the five calls above (bf_smpl_forward, bf_smpl_vjp, bf_smplx_forward[_expr], bf_smplx_vjp[_expr],
 * bf_keypoint_loss) on DEVICE pointers, ordered on the caller's stream.  For a caller whose arrays live on the GPU already and
 * who shares this library's HIP runtime - a torch process that imported torch before the library was loaded, so that the
 * loader resolved both to one libamdhip64; bf_device_pointer_check is how to find out.  In a process with two runtimes
 * pointers and streams must not cross: use the host entry points.
 *
 * Every *_dev call issues its host twin's kernels, in its order, with its grids and arguments - equal inputs give the host
 * twin's bits - on `stream` (a hipStream_t; NULL = the null stream) and returns when the work is queued.  It calls no
 * hipDeviceSynchronize, hipStreamSynchronize, blocking hipMemcpy, hipMalloc or hipFree, except: a workspace buffer that has to
 * grow (the first call of a shape), the model's transposed pose directions built by the first reverse call (complete on the
 * device before that call returns), and a `divisor` that differs from the one sent last.  Every array is a contiguous float32
 * (dyn_row: int32) device pointer on the model's device and must stay alive until `stream` reaches the end of the call.  NULL
 * keeps its meaning (an output not wanted, a cotangent of zero).  Bad arguments fail before anything is queued, with the host
 * twin's refusals.
 *
 * A workspace owns the scratch of ONE caller: grow-only device buffers and one event.  One call at a time per workspace (the
 * caller locks).  A buffer grows only when a call needs more than it holds, after the stream it was last used on has
 * drained; a second call of the same shapes allocates nothing and waits for nothing.  A call on another stream than the
 * workspace's previous call first makes its stream wait for the event recorded at the end of that call.
 * bf_workspace_destroy drains the last stream before it frees.  The device's block cache is not used on this route. */
typedef struct bf_workspace bf_workspace;
int bf_workspace_create(int device, bf_workspace **out);
void bf_workspace_destroy(bf_workspace *ws);
int bf_smpl_forward_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const float *betas, const float *global_orient,
                        const float *body_pose, float *vertices, float *joints, float *joints_ori);
int bf_smpl_vjp_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const float *betas, const float *global_orient,
                    const float *body_pose, const float *dvertices, const float *djoints, const float *djoints_ori,
                    float *dbetas, float *dglobal_orient, float *dbody_pose);
/* the structs of the host calls, holding device pointers; expression NULL = the call without coefficients */
int bf_smplx_forward_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const bf_smplx_params *in, const float *expression,
                         const bf_smplx_outputs *out);
int bf_smplx_vjp_dev(bf_model *m, bf_workspace *ws, void *stream, int n, const bf_smplx_params *in, const float *expression,
                     const bf_smplx_cotangents *cot, const bf_smplx_grads *grads, float *dexpression);
/* bf_keypoint_loss_in with device pointers, except `divisor`: a HOST array of n ints, validated on the host and sent by the
 * call.  The device is the GMM's, which must be the workspace's; without a GMM the workspace's. */
int bf_keypoint_loss_dev(bf_workspace *ws, void *stream, const bf_gmm *gmm, const bf_keypoint_loss_in *in, const bf_hyper *hyper,
                         const float *dterms, float *terms, float *djoints, float *dposes, float *dbetas);
/* BF_OK when this library's HIP runtime knows `p` as device memory of `device`, else BF_ERR_INVALID (NULL, host memory, memory
 * of another runtime or device).  Never sets bf_last_error and leaves no HIP error behind. */
int bf_device_pointer_check(int device, const void *p);
/* test hook, process-wide counts: out[0] calls of the five host entry points named above, of the SMPL+D stage's losses below
 * (bf_vertex_normals, bf_vertex_normals_vjp, bf_normal_laplacian, bf_scan_point_loss, bf_normal_loss), of bf_scan_nearest, of bf_silhouette_loss and of bf_nr_render[_taped], bf_nr_tape_texture_grad, bf_nr_tape_vertex_grad,
 * out[1] calls of the *_dev entry points (both counted once the arguments have passed), out[2] device (re)allocations of workspaces, out[3] calls that had to wait
 * for their workspace's previous call on another stream. */
int bf_dev_route_stats(int64_t out[4]);

/* The SMPL+D stage's losses (smplify.py:236-245) as stand-alone calls with their gradients, for a user's own torch loop: what
 * bf_fit_displacement evaluates fused, one mesh per call.  Host pointers; the calls' buffers come from the device's block cache;
 * no float atomics, every scalar is reduced in one order that depends on the sizes alone, so equal inputs give equal bits.
 * At most 2^28 vertices, faces or points (BF_ERR_UNSUPPORTED beyond).
 *
 * A mesh topology on one device, uploaded once: faces[n_faces,3] and the vertex -> (face, corner) lists in the order
 * compute_normal_torch (utils/io_utils.py:406-428) adds a vertex's face normals up - corner by corner, faces ascending.  A face
 * index outside [0, n_verts) is BF_ERR_INVALID. */
typedef struct bf_topo bf_topo;
int bf_topo_create(int device, int n_verts, int n_faces, const int32_t *faces, bf_topo **out);
void bf_topo_destroy(bf_topo *t);
/* compute_normal_torch: verts[n_verts,3] -> normals[n_verts,3]; face normals n / (|n| + 1e-8), summed per vertex, divided by
 * (|sum| + 1e-8) again.  A vertex in no face gets exactly zero. */
int bf_vertex_normals(const bf_topo *t, const float *verts, float *normals);
/* ... and its vector-Jacobian product: dverts[n_verts,3] = the gradient of sum(dnormals * normals), dnormals[n_verts,3] any
 * cotangent.  Where a length is zero torch's rule holds (d = dn / 1e-8, no projection term). */
int bf_vertex_normals_vjp(const bf_topo *t, const float *verts, const float *dnormals, float *dverts);
/* normal_laplacian_smoothness (smplify/loss.py:273-288): loss[1] = mean over faces of |na-nb|^2 + |nc-na|^2 + |nb-nc|^2 of
 * norms[n_verts,3]; dnorms[n_verts,3] = its gradient for cotangent 1.  Either output may be NULL = not wanted. */
int bf_normal_laplacian(const bf_topo *t, const float *norms, float *loss, float *dnorms);
/* point_cloud_loss_mesh_grid (smplify/loss.py:233-242): bf_scan_nearest's launch for points[n,3], then loss[1] = sqrt(sum
 * |P - C|^2) over all points with the closest points C detached, and dpoints[n,3] = (P - C) / loss for cotangent 1 - exactly zero
 * where the loss is zero.  face_ids[n] and nearest[n,3] are bf_scan_nearest's.  Every output may be NULL = not wanted. */
int bf_scan_point_loss(bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints);
/* normal_loss_mesh_grid (smplify/loss.py:260-271) behind the search: closest_face_norms[n,3] = face_norm_mesh[closest face]
 * (gathered by the caller, un-normalised as smplify.py:149 builds them), point_norms[n,3] -> loss[1] = mean(1 - sum(fn * pn)),
 * dpoint_norms[n,3] = -fn / n for cotangent 1.  Either output may be NULL = not wanted. */
int bf_normal_loss(int device, int n, const float *closest_face_norms, const float *point_norms, float *loss, float *dpoint_norms);

/* The device route of the calls above and of bf_scan_nearest (see bf_workspace): the twin's arguments as DEVICE pointers, then the
 * workspace and the stream (a hipStream_t; NULL = the null stream).  Each issues its twin's kernels in its twin's order, with its
 * grids and arguments, on `stream` - equal inputs give the twin's bits - writes its results through the caller's pointers and
 * returns when the work is queued: no drain, no copy to the host.  A scalar loss is ONE float in device memory.  Scratch (face
 * normals, partial sums, an output not wanted) comes from the workspace, which must live on the topology's / scan's device
 * (BF_ERR_INVALID otherwise, as for a NULL workspace).  The first *_dev call on a scan puts the scan's descriptor into device
 * memory, once, complete before that call returns.  Bad arguments fail before anything is queued, with the twin's refusals; the
 * thread's current device is left as it was.  NULL outputs keep the twin's meaning. */
int bf_vertex_normals_dev(const bf_topo *t, const float *verts, float *normals, bf_workspace *ws, void *stream);
int bf_vertex_normals_vjp_dev(const bf_topo *t, const float *verts, const float *dnormals, float *dverts, bf_workspace *ws, void *stream);
int bf_normal_laplacian_dev(const bf_topo *t, const float *norms, float *loss, float *dnorms, bf_workspace *ws, void *stream);
int bf_scan_point_loss_dev(bf_scan *s, int n, const float *points, float *loss, int32_t *face_ids, float *nearest, float *dpoints,
                           bf_workspace *ws, void *stream);
/* bf_scan_nearest (no warm start): face_ids[n], nearest[n,3], bary[n,3], each may be NULL = not wanted */
int bf_scan_nearest_dev(bf_scan *s, int n, const float *points, int32_t *face_ids, float *nearest, float *bary, bf_workspace *ws,
                        void *stream);
/* bf_normal_loss with the gather inside the kernel: face_ids[n] = the closest faces (bf_scan_point_loss_dev's or
 * bf_scan_nearest_dev's), face_norm_table[n_faces,3] = the caller's whole face_norm_mesh; the bits are bf_normal_loss's on
 * face_norm_table[face_ids].  An id outside [0, n_faces) is not dereferenced: its row adds 0 to the sum (the mean still divides by
 * n) and its dpoint_norms row is zero. */
int bf_normal_loss_dev(int device, int n, const int32_t *face_ids, const float *face_norm_table, int n_faces, const float *point_norms,
                       float *loss, float *dpoint_norms, bf_workspace *ws, void *stream);
/* The backward of a scalar loss without reading the cotangent back: out[n] = grad[n] * cotangent[0] in float32, plus_zero != 0:
 * + 0.0f behind the product (a zero is +0 whatever the cotangent's sign).  All three are device pointers of `device`; out may be
 * grad.  One launch on `stream`, no workspace. */
int bf_scale_gradient_dev(int device, int n, const float *grad, const float *cotangent, int plus_zero, float *out, void *stream);

/* The model's forward for `n` packed parameter vectors params[n,n_params] (any model kind): vertices[n,NV,3] in
 * model space and joints[n,n_joint_map,3], both before the similarity (either may be NULL). */
int bf_model_forward(bf_model *m, int n, const float *params, float *vertices, float *joints);

/* One batch = F frames that SMPLify.__call__ (smplify.py:84-250) would process one after another
 * (apps/genebody_fitting.py:183-192), each with V calibrated views. */
int bf_batch_create(bf_model *m, int n_frames, int n_views, bf_batch **out);
void bf_batch_destroy(bf_batch *b);

/* c2w[F,V,4,4], K[F,V,3,3]: what the caller passes as `c2ws`, `Ks` (smplify.py:84); inverted to
 * world-to-camera here (smplify.py:131-135). */
int bf_batch_set_cameras(bf_batch *b, const float *c2w, const float *K);
/* keypoints[F,V,n_loss_joints,3] = (x, y, confidence): keypoints[i]['pose'] of loss.py:160.  A view
 * without a detection (None, loss.py:157) is passed with all confidences 0.  n_use_frames[F] is the
 * divisor len(use_frames) of loss.py:197 (NULL -> V). */
int bf_batch_set_keypoints(bf_batch *b, const float *keypoints, const int32_t *n_use_frames);
/* init_betas[F,NB], init_pose[F,72] = net_output of smplify.py:103 (SMPL-X takes [:, 3:66] as body pose,
 * :110-112; eyes / hand PCA start at 0, :118-122); transl=0, scale=1 (:126-128) */
int bf_batch_set_init(bf_batch *b, const float *init_betas, const float *init_pose);
/* The NEXT frame's keypoints[F,V,n_loss_joints,3], n_use_frames[F] (NULL -> V), init_betas[F,NB], init_pose[F,72] (layouts of
 * bf_batch_set_keypoints / bf_batch_set_init) without waiting for the work in flight: the frame loop of
 * apps/genebody_fitting.py:183-192 hands SMPLify.__call__ new detections and a new HMR estimate every frame (and loss.py:160
 * uploads the keypoints again every iteration).  The arrays are copied into pinned staging before the call returns; their
 * transfer into the device arena the running fit does not read is queued behind that fit on the batch's stream - or, in the
 * frame-after-frame loop (fits with BF_FIT_RESET | BF_FIT_FETCH | BF_FIT_NOTIME), on the batch's second stream, where it runs
 * UNDER the fit in flight (round 5; the fit that reads it waits for it, on the host).  The next bf_fit must carry
 * BF_FIT_RESET (anything else fails with BF_ERR_INVALID).  Cameras, masks and scans are not staged: they stay as set. */
int bf_batch_stage_inputs(bf_batch *b, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose);
/* Re-arm the batch for another fit of the same inputs without touching the host: restores the
 * parameters of the last bf_batch_set_init / bf_batch_set_params and clears the Adam state, as
 * stream-ordered device copies.  (The reference rebuilds everything per frame, body_fitting.py:82.) */
int bf_batch_reset(bf_batch *b);
/* direct access to the packed optimised scalars [F,n_params] (for stage-level tests / warm starts) */
int bf_batch_set_params(bf_batch *b, const float *params);
int bf_batch_get_params(bf_batch *b, float *params);

/* The optimisation loop smplify.py:177-213: n_iters Adam steps on every frame.  Asynchronous. */
int bf_fit(bf_batch *b, int n_iters, const bf_hyper *hyper, uint32_t flags);
/* One evaluation of multiview_keypoint_loss (loss.py:139-230) and its gradient at the current
 * parameters, no update: terms[F,4] = reprojection, pose_prior, angle_prior, shape_prior
 * (loss.py:219-224); grads[F,n_params]. */
int bf_loss_grad(bf_batch *b, const bf_hyper *hyper, float *terms, float *grads);
/* The gradient one dense iteration of bf_fit hands to Adam, read without taking the step (a test hook, like bf_loss_grad).
 * At the batch's current parameters it runs that iteration's passes one launch after the other (pose state, forward mesh,
 * keypoint / silhouette / scan losses, reverse mesh pass, reduction - the schedule bf_fit uses when the fit kernel is not
 * resident) and then the fit kernel without its update.
 *   flags  BF_DENSE_GRAD_LATE: the iteration is one after the switch-on (smplify.py:197,205): the silhouette and scan terms are
 *          on with bf_fit's weights, 5 and 5 * imsize / scan_height.  With neither scans nor silhouettes attached: BF_ERR_INVALID.
 *          BF_DENSE_GRAD_SUBMODEL: the mesh passes run on the sub-model bf_fit would choose for such an iteration (none where
 *          bf_fit would use the full model: then the flag changes nothing); without it they run on the full model.
 *   dverts_extra[F,NV,3] (host, the full model's vertex order; may be NULL) is added onto dL/d(body vertices) just before the
 *          reverse mesh pass, at the vertices that pass runs on: the objective becomes L + sum(dverts_extra * body_vertices).
 *   terms[F,6] = reprojection, pose_prior, angle_prior, shape_prior (as bf_loss_grad), 5 x silhouette loss,
 *          5 * imsize / scan_height x point-cloud loss; the last two are 0 without BF_DENSE_GRAD_LATE (or with nothing of their
 *          kind attached).  grads[F,n_params].  Either may be NULL.
 * With flags 0 and no dverts_extra, grads are bf_loss_grad's bit for bit: SMPL-kind models, whose keypoint loss the fit kernel
 * computes itself, then take the plain fit launch bf_fit uses for such an iteration, without a mesh pass.  (Through the mesh
 * passes - a dverts_extra, even of zeros - the sized SMPL instance of the fit kernel sums dL/dbetas in another order than its plain
 * instance: equal to rounding, not to the bit.)  The silhouette's projection runs as a launch of its own here (bf_fit folds it into
 * the forward mesh pass; the arithmetic is shared).
 * Synchronous.  Parameters, Adam state, the step count and the closest-point search's warm start stay as they were: a bf_fit
 * continued afterwards gives the bits it would have given without the call.  The vertices / joints / loss terms that
 * bf_batch_get_result reads on the device are overwritten (results already fetched with BF_FIT_FETCH are not).
 * A batch whose scan was destroyed, or whose next inputs are staged, is refused with BF_ERR_INVALID, as by bf_fit. */
#define BF_DENSE_GRAD_LATE     1u
#define BF_DENSE_GRAD_SUBMODEL 2u
int bf_dense_iter_grad(bf_batch *b, const bf_hyper *hyper, uint32_t flags, const float *dverts_extra, float *terms, float *grads);
int bf_batch_sync(bf_batch *b);

/* rtn_dict of smplify.py:216-226 after bf_fit (any pointer may be NULL):
 * vertices[F,NV,3], joints[F,n_joint_map,3], full_pose[F,3NJ] come from the LAST forward pass
 * (parameters before the final step, as in the reference); the stepped parameters come from
 * bf_batch_get_params.  loss_terms[F,4] are those of the last evaluated iteration. */
int bf_batch_get_result(bf_batch *b, float *vertices, float *joints, float *full_pose, float *loss_terms);
/* The result of the fit issued BEFORE the last one, without waiting for the last one: with bf_batch_stage_inputs this makes the
 * frame loop a two-deep pipeline (frame i's rtn_dict, smplify.py:216-226, is read while frame i+1 is being fitted).  Both fits
 * must have been issued with BF_FIT_RESET | BF_FIT_FETCH | BF_FIT_NOTIME on the keypoint-only path - their results then sit in
 * the batch's two result arenas.  params[F,n_params] + the outputs of bf_batch_get_result; any pointer may be NULL. */
int bf_batch_get_previous(bf_batch *b, float *params, float *vertices, float *joints, float *full_pose, float *loss_terms);
/* packed [F,n_params] stepped parameters copied into a DEVICE buffer (e.g. the send buffer of the
 * final RCCL all-gather when frames are sharded over GPUs) */
int bf_batch_export_params_dev(bf_batch *b, void *dst_dev);

/* ---- scan closest-point path (use_mesh, BASELINE config 5) ------------------------------------------
 * MeshGridSearcher(verts, faces) (utils/mesh_grid_searcher.py:51-79 -> insert_grid_surface,
 * thirdparty/mesh_grid/mesh_grid.cpp:31-52): verts[n_verts,3], faces[n_faces,3] int32. */
/* ORDER OF DESTRUCTION: a scan may be destroyed while batches still hold it (bf_batch_set_scans): bf_scan_destroy then waits for
 * the device and DETACHES every scan from those batches, which are marked: their next bf_fit / bf_fit_displacement returns
 * BF_ERR_INVALID ("a scan this batch held was destroyed") until a bf_batch_set_scans call succeeds - with NULL to go on without
 * scans; a call that is rejected leaves the mark (rounds 4-5 let the fit run silently without the closest-point loss).  A batch may be destroyed before its scans.
 * Not thread-safe against a bf_fit / bf_batch_set_scans of a holding batch running at the same moment on another thread.
 * bf_scan_create builds the grid on the NULL stream and waits for that stream only (the library's streams are non-blocking):
 * a fit in flight on a batch's stream keeps running. */
int bf_scan_create(int device, int n_verts, const float *verts, int n_faces, const int32_t *faces, bf_scan **out);
void bf_scan_destroy(bf_scan *s);
float bf_scan_height(const bf_scan *s);                 /* (max - min)[1], smplify.py:150-151 */
/* The library caches the device blocks of destroyed scans per device (at most 2 GB; a failed hipMalloc empties it and retries):
 * give them back to the runtime now.  -> bytes released, < 0 on a bad device index.  (Waits for the device, as hipFree does.) */
int64_t bf_device_cache_trim(int device);
int bf_scan_grid_info(const bf_scan *s, int32_t dims[3], float origin_step[4]);
/* The tensors insert_grid_surface leaves with its caller (mesh_grid.cpp:129-136, mesh_grid_kernel.cu:178-236; built on
 * the device by bf_scan_create): tri_num[nx*ny*nz] = inclusive cumulative triangle count per cell (cell = (x*ny+y)*nz+z),
 * tri_idx[*n_entries] = face id + 1 per list entry, ascending inside a cell (the reference's order inside a cell is
 * whatever its atomicCAS race produced).  Any pointer may be NULL; call once with tri_idx NULL to learn n_entries. */
int bf_scan_grid_lists(const bf_scan *s, int32_t *tri_num, int32_t *tri_idx, int32_t *n_entries);
/* MeshGridSearcher.nearest_points / search_nearest_point (mesh_grid.cpp:54-72): points[n,3] ->
 * face_ids[n] int32, nearest[n,3], bary[n,3] (any output may be NULL) */
int bf_scan_nearest(bf_scan *s, int n, const float *points, int32_t *face_ids, float *nearest, float *bary);
/* The same search with a guess per query, hint[n,3] (NULL: none) = where the nearest point is believed to be - the fit loop hands the
 * search its previous iteration's answer this way.  The guess bounds the search and is CHECKED against what was found (searched again
 * without it when it was wrong): the results are bf_scan_nearest's for any hint.  reps > 0 with kernel_us != NULL: the launch is repeated
 * and its mean device time returned (microseconds). */
int bf_scan_nearest_hinted(bf_scan *s, int n, const float *points, const float *hint, int32_t *face_ids, float *nearest, float *bary,
                           int reps, float *kernel_us);
/* The per-triangle arithmetic of every closest-point search of the process (bf_scan_nearest, the scan loss of bf_fit, SMPL+D).
 * BF_NEAREST_REFERENCE (default): search_nearest_proj as the reference's source evaluates it in float32 - Gram matrix of the corner
 * vectors, the bordered 4 x 4 system through solve4 / solve3 with their pivot order and absolute 1e-9 rank tests, IEEE divisions,
 * no fused multiply-adds (mesh_grid_kernel.cu:12-109, matrix.h:13-316): face ids, coefficients and points are those of the
 * reference's arithmetic wherever no two faces return the same distance bit for bit (such ties go to the lowest face id; the
 * reference's own order inside a cell is an atomicCAS race).  BF_NEAREST_FAST: the same rule through the 2 x 2 normal equations
 * and v_rcp_f32 - about half the instructions, other last bits (DESIGN.md 2.3 has the measured difference).
 * Also read once from the environment: BF_NEAREST_RULE=reference|fast. */
#define BF_NEAREST_REFERENCE 0
#define BF_NEAREST_FAST      1
int bf_nearest_rule_set(int rule);                     /* 0 on success, -1 for an unknown rule */
int bf_nearest_rule_get(void);
/* How the silhouette loss's contour gradients (loss.py:110-119: every contour point pulls its nearest projected vertex) reach
 * dL/dvertices inside bf_fit.  BF_MASK_FOLD_SUMS (default, round 5): the contour scan adds each point's pull onto its vertex as a
 * 64-bit fixed-point number (steps of 2^-40, exact sums: the order of the atomic additions does not matter, so a fit is reproducible
 * bit for bit) and the reverse mesh pass maps the sums back through the projection.  BF_MASK_FOLD_GATHER: the ordered walk of
 * rounds 2-4 (bf_mask_gather_kernel: a vertex adds its contour points up in contour order, in float32) - one more launch per
 * iteration, last bits of the sum differ.  bf_batch_mask_loss always takes the ordered walk.
 * Also read once from the environment: BF_MASK_FOLD=sums|gather. */
#define BF_MASK_FOLD_SUMS   0
#define BF_MASK_FOLD_GATHER 1
int bf_mask_fold_set(int mode);                        /* 0 on success, -1 for an unknown mode */
int bf_mask_fold_get(void);
/* Self-tests of the reference-arithmetic rule: out[i] = num[i] / den[i] through the kernel's division helper (exact IEEE division
 * for 1e-8 < |den| < 4, |num / den| < 2^90); the per-triangle rule itself on patches[n][9] = the corners relative to the query
 * (mesh_grid_kernel.cu:305-311) -> dist[n], coeff[n][3]; general = 0 evaluates the straight-line paths alone and returns -1 where
 * they decline. */
int bf_nearest_selftest_quot(int device, int n, const float *num, const float *den, float *out);
int bf_nearest_selftest_rule(int device, int n, const float *patches, int general, float *dist, float *coeff);
/* SurfaceNearest.backward with respect to the query points (utils/mesh_grid_searcher.py:17-49; search_nearest_point_backward,
 * mesh_grid.cpp:120-128, mesh_grid_kernel.cu:354-382 - left unfinished in the reference: its kernel never inverts the KKT matrix).
 * face_ids[n], bary[n,3] as bf_scan_nearest returned them, dnearest[n,3] = dL/d(nearest point) -> dpoints[n,3] = dL/d(query):
 * the projection onto the plane (I - n n^T), the edge (d d^T / |d|^2) or the corner (0) the closest point lies on. */
int bf_scan_nearest_backward(bf_scan *s, int n, const int32_t *face_ids, const float *bary, const float *dnearest, float *dpoints);
/* MeshGridSearcher.inside_mesh / search_inside_mesh (utils/mesh_grid_searcher.py:86-91, mesh_grid.cpp:74-90,
 * mesh_grid_kernel.cu:569-641): signs[n] = +1 inside (odd number of triangles crossed by the axis ray towards the
 * nearest grid wall), -1 outside or off the grid. */
int bf_scan_inside(bf_scan *s, int n, const float *points, float *signs);
/* MeshGridSearcher.intersects_any / search_intersect (utils/mesh_grid_searcher.py:93-99, mesh_grid.cpp:92-110,
 * mesh_grid_kernel.cu:742-1026,1029-1231): hit[n] = 1 when the ray origins[i] + t directions[i], t >= 0, meets a triangle by the
 * reference's per-triangle test intersect_tri2, its branches for rays inside a triangle's plane and for degenerate triangles included. */
int bf_scan_intersects(bf_scan *s, int n, const float *origins, const float *directions, uint8_t *hit);
/* use_mesh=True: scans[F], one per frame (NULL detaches).  Sets each frame's constant scale to
 * scan_height / 1.7 (smplify.py:156); bf_fit then adds 5 * point_cloud_loss / scan_height * imsize for
 * iterations i > n_iters // 3 (smplify.py:205-210). */
int bf_batch_set_scans(bf_batch *b, bf_scan *const *scans);
/* ---- silhouette loss (use_mask, BASELINE config 3) ----------------------------------------------------
 * masks[F,M,H,W] uint8 as loaded (> 128 = foreground, smplify.py:139); view_index[M] = position of each mask
 * view among the V views (smplify.py:141-142); per (frame, mask view) contour_count[F*M] contour points,
 * concatenated as (x, y) pairs in contour_xy (what extract_countours returns, loss.py:73-83).  bf_fit then
 * adds 5 * multview_mask_loss for iterations i > n_iters // 3 (smplify.py:197-199,210).  n_masks = 0 detaches. */
/* contour_count == NULL (and contour_xy == NULL): the contours are extracted from the masks on the device - Suzuki-Abe
 * border following = cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) - and ONE external border per mask is kept, chosen by
 * contour_select (ignored when the caller passes contours).  The reference keeps
 * `contour[np.argmax([a.shape[1] for a in contour])]` (loss.py:80); every OpenCV contour has shape [C,1,2], so the argmax
 * runs over ones and returns OpenCV's FIRST listed contour.  OpenCV lists external borders in the reverse of the order its
 * raster scan meets them (each new contour is inserted as the first child of the frame), so that is the border whose start
 * pixel comes LAST in raster order: BF_CONTOUR_OPENCV_FIRST, the default.  For a one-component silhouette all three coincide.
 * In this form the call returns once the mask upload and the border following are QUEUED (on the batch's second stream); the
 * next bf_fit / bf_batch_mask_loss collects the contours right before the first kernel that reads them - in a fit, under the
 * iterations that need no silhouette yet.  The caller's `masks` buffer is copied before the call returns. */
#define BF_CONTOUR_OPENCV_FIRST 0   /* the last external border the raster scan meets = contours[0] of OpenCV = what loss.py:80 keeps */
#define BF_CONTOUR_RASTER_FIRST 1   /* the first external border the raster scan meets */
#define BF_CONTOUR_LONGEST      2   /* the longest external border (first on ties): the evident intent of loss.py:80 */
int bf_batch_set_masks(bf_batch *b, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks,
                       const int32_t *contour_count, const float *contour_xy, int contour_select);
/* The NEXT frame's silhouettes without draining the work in flight (a capture hands SMPLify new masks with every frame,
 * apps/genebody_fitting.py:183-192; smplify.py:138-144): same views and image shape as the masks attached with bf_batch_set_masks
 * (contour_count = NULL there: contours on the device).  Binarisation, upload and border following (loss.py:73-83) go into a second
 * arena, on the batch's second stream, under the fit in flight; the next bf_fit uses them.  Two-deep: the call waits for the fit that
 * last read the arena it overwrites. */
int bf_batch_stage_masks(bf_batch *b, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks, int contour_select);
/* extract_countours (smplify/loss.py:73-83) on its own: masks[n,H,W] uint8 (non-zero = foreground) -> counts[n] and,
 * when xy != NULL, the (x, y) points of the n contours concatenated (sum(counts) pairs; call with xy == NULL first). */
int bf_extract_contours(int device, int n, int H, int W, const uint8_t *masks, int32_t *counts, float *xy, int select);
/* one evaluation of multview_mask_loss (loss.py:85-130) at the current parameters: loss[F] and its gradient
 * w.r.t. body_vertices, dverts[F,NV,3] (either may be NULL) */
int bf_batch_mask_loss(bf_batch *b, const bf_hyper *hyper, float *loss, float *dverts);

/* multview_mask_loss (smplify/loss.py:85-130) on vertices the CALLER holds - their own model's, SMPL+D displaced ones, the drop-in
 * SMPL's with their own similarity - for a user's own torch loop (smplify.py:198): no model and no batch behind it.
 *
 * A silhouette object = the M views' masks[M,H,W] (uint8, non-zero = foreground) and one contour per view, on one device for the
 * object's life.  contour_count == NULL: the external borders are followed on the device, as bf_batch_set_masks does it, and the
 * one contour_select names is kept (BF_CONTOUR_*).  Otherwise contour_count[M] points per view, concatenated as (x, y) pairs in
 * contour_xy (contour_select is not read); a view may have no points - it then contributes its binary term only.
 * Limits (BF_ERR_UNSUPPORTED beyond): M <= 65535 (a grid dimension), H, W <= 16384 (pixel coordinates and H * W stay exact in
 * float32 / int), a contour of at most BF_SIL_MAX_CONTOUR = 2^22 points (16 lanes per point in an int).  The object is used by
 * one thread at a time. */
#define BF_SIL_MAX_VIEWS   65535
#define BF_SIL_MAX_SIDE    16384
#define BF_SIL_MAX_CONTOUR (1 << 22)
typedef struct bf_silhouette bf_silhouette;
int bf_silhouette_create(int device, int n_views, int H, int W, const uint8_t *masks, const int32_t *contour_count,
                         const float *contour_xy, int contour_select, bf_silhouette **out);
void bf_silhouette_destroy(bf_silhouette *s);
/* The contours the object holds: counts[M] and, when xy != NULL, their (x, y) points concatenated (sum(counts) pairs; call with
 * xy == NULL first), as bf_extract_contours. */
int bf_silhouette_contours(const bf_silhouette *s, int32_t *counts, float *xy);
/* One evaluation on the sampled vertices verts[::stride] (ceil(n_verts / stride) of them; the reference hard-codes 4) of
 * verts[n_verts,3], with cameras w2c[M,4,4] (rows 0..2 are read) and K[M,3,3]:
 *   per view  pixels = K (R x + t) / z, no epsilon on the depth; inside = 0 <= u, v < imsize;
 *     contour term  sum over the contour's points of w * the distance to the nearest inside vertex (first minimum, as torch.min
 *                   picks it), w = epsilon where the mask is < 0.1 at that vertex's truncated pixel, else 1; a view with no
 *                   inside vertex has contour term exactly 0;
 *     binary term   epsilon * sum over ALL sampled vertices of bilinear(1 - mask) at the pixel normalised by imsize (grid_sample,
 *                   zeros padding, align_corners=False).
 * cdist_form != 0: distances as torch.cdist computes them in float32 (what the reference computes): its expanded form -
 * bf_hyper.mask_cdist_form's - in a view with more than 25 inside vertices, direct (a - b)^2 sums in a view with fewer, where
 * torch does not switch to the expanded form either; 0: direct sums everywhere.
 * loss[1] = the unweighted value, as the function returns it; view_terms[M,2] = per view (contour term, binary term); loss is
 * their float32 sum taken in memory order (view 0's contour term, view 0's binary term, view 1's ...).  dverts[n_verts,3] = the
 * gradient for cotangent 1, exactly zero (every bit) at vertices that are not sampled.  Every output may be NULL = not wanted.
 * Three launches and one read-back per call.  No float atomics: the contour term's gradient is summed as 64-bit fixed-point
 * numbers (exact, so order-free), everything else in a fixed order - equal inputs give equal bits, and a view's view_terms row
 * and its share of dverts do not depend on which other views are in the call.
 * The fixed-point sums hold steps of 2^-40 in 63 bits: a call with max(|epsilon|, 1) * (longest contour) > BF_SIL_MAX_SUM = 2^20
 * (|sum| 2^60 at most: a factor of 8 below the overflow) is REFUSED with BF_ERR_UNSUPPORTED - there is no second, ordered path.
 * BF_ERR_INVALID, before any launch: n_verts < 1, stride < 1, imsize or epsilon not finite, imsize <= 0; more than 2^28
 * vertices: BF_ERR_UNSUPPORTED. */
#define BF_SIL_MAX_SUM (1 << 20)
int bf_silhouette_loss(bf_silhouette *s, int n_verts, int stride, const float *verts, const float *w2c, const float *K,
                       float imsize, float epsilon, int cdist_form, float *loss, float *view_terms, float *dverts);

/* The device route of the silhouette term (see bf_workspace): extract_countours and multview_mask_loss (smplify/loss.py:73-130)
 * for a caller whose masks, vertices and cameras are DEVICE arrays of this library's HIP runtime, ordered on `stream` (a
 * hipStream_t; NULL = the null stream).  Each call counts as a *_dev call in bf_dev_route_stats, bf_silhouette_loss as a host call.
 *
 * bf_silhouette_create_dev: masks[M,H,W] contiguous on `device`, one byte per pixel (BF_MASK_UINT8: uint8 or bool) or float32
 * (BF_MASK_FLOAT32), aligned to its element and no further; it may still be in flight on `stream`.  One launch there reads the
 * masks in their type, writes the object's 0 / 1 bytes and raises M + 1 flags; the call waits for `stream` and reads the flags -
 * the pixels never cross to the host.  A value other than 0 / 1 (a NaN is one): BF_ERR_INVALID.  A view with no foreground: the
 * POSITIVE return value BF_SIL_EMPTY_VIEW + the first such view's index, and no object.  Otherwise the contours are followed as
 * by bf_silhouette_create(contour_count = NULL): the same storage, contours and limits.  Creation synchronises; it happens once
 * per masks object.  The thread's current device is left as it was. */
#define BF_MASK_UINT8      0
#define BF_MASK_FLOAT32    1
#define BF_SIL_EMPTY_VIEW  1
int bf_silhouette_create_dev(int device, int n_views, int H, int W, const void *masks, int mask_dtype, int contour_select,
                             void *stream, bf_silhouette **out);
/* The contours' (x, y) points, sum(counts) pairs (counts: bf_silhouette_contours(s, counts, NULL)), copied device to device
 * into xy on `stream`. */
int bf_silhouette_contours_dev(const bf_silhouette *s, float *xy, void *stream);
/* bf_silhouette_loss on device arrays: verts[n_verts,3], w2c[M,4,4], K[M,3,3] float32 on the object's device.  terms[1 + 2M] =
 * the loss, then view_terms[M,2]; dverts[n_verts,3]; either may be NULL = not wanted, with both NULL nothing is launched.  The
 * rows K [R|t] are formed by a launch of their own, in double, with the host call's bits; then the host call's three launches
 * with its grids and arguments - equal inputs give its bits.  Scratch comes from the workspace, which must live on the object's
 * device (BF_ERR_INVALID otherwise, as for a NULL one); no memset, no copy to the host, no drain.  The host call's refusals,
 * before anything is queued; the thread's current device is left as it was. */
int bf_silhouette_loss_dev(bf_silhouette *s, int n_verts, int stride, const float *verts, const float *w2c, const float *K,
                           float imsize, float epsilon, int cdist_form, float *terms, float *dverts, bf_workspace *ws, void *stream);
/* TEST HOOK, not part of the feature: that first launch by itself, so that bf_sil_rows_kernel can be held to the float64 expression
 * on its own (the loss's outputs do not allow it).  rows[M,3,4] = K [R|t] from w2c[M,4,4] and K[M,3,3], device pointers of `device`; each element is
 * (float)((double)k0 * w0 + (double)k1 * w1 + (double)k2 * w2) summed left to right - a product of two float32 values is exact in
 * double, so the bits do not depend on whether a multiply-add is fused.  One launch on `stream`, no workspace. */
int bf_silhouette_rows_dev(int device, int n_views, const float *w2c, const float *K, float *rows, void *stream);

/* SMPL+D stage (displacement=True, smplify.py:228-247): n_iters Adam steps (lr 5e-2) on a per-vertex
 * displacement of the vertices returned by the last bf_fit, against each frame's scan:
 * loss = icp + (normal_loss + laplacian) * constant_scale * 0.1.  Needs faces in the model and scans. */
int bf_fit_displacement(bf_batch *b, int n_iters, const bf_hyper *hyper);
int bf_batch_get_displacement(bf_batch *b, float *displacement /*[F,NV,3]*/);


/* ---- frames sharded over the GPUs of one node (BASELINE config 4 / 5) -----------------------------------
 * Replaces the serial `for frame` loop of apps/genebody_fitting.py:183-192: frames are independent, so frame f goes to
 * shard f // ceil(F / n) in contiguous blocks, model and cameras are replicated, nothing is exchanged during the fit, and
 * the fitted parameters are all-gathered ONCE over RCCL (xGMI) at the end.  No PyTorch on this path; librccl is opened
 * lazily the first time a communicator is needed. */
/* host arithmetic, no device: the partition (blocks differ by at most one frame), the per-shard capacity the all-gather is
 * padded to, and the unpacking of a gathered [n_shards][capacity][width] block into [n_frames][width] */
int bf_shard_range(int n_frames, int n_shards, int shard, int32_t *first, int32_t *count);
int bf_shard_capacity(int n_frames, int n_shards);
int bf_shard_unpack(const float *gathered, int n_frames, int n_shards, int width, float *out);
/* block starts of the silhouette contours (bf_batch_set_masks' contour_count[n_frames * n_masks] / contour_xy) per shard:
 * xy_first[n_shards + 1] = (x, y) pairs in front of every shard's first contour, then their total */
int bf_shard_contour_offsets(int n_frames, int n_shards, int n_masks, const int32_t *contour_count, int64_t *xy_first);

/* ONE process driving n devices: a bf_model + bf_batch + stream per device (devices == NULL -> 0..n-1),
 * ncclCommInitAll on first use.  The setters take the arrays of the whole job [F, ...] (layouts of the bf_batch_set_*
 * counterparts) and hand every device its block; bf_group_fit queues bf_fit on every device and returns. */
typedef struct bf_group bf_group;
int bf_group_create(const bf_model_desc *desc, int n_devices, const int32_t *devices, int n_frames, int n_views, bf_group **out);
void bf_group_destroy(bf_group *g);
int bf_group_n_devices(const bf_group *g);
int bf_group_n_params(const bf_group *g);
int bf_group_shard(const bf_group *g, int i, int32_t *device, int32_t *first, int32_t *count);
bf_batch *bf_group_batch(bf_group *g, int i);      /* device i's block as an ordinary batch (masks, scans, results, timing) */
bf_model *bf_group_model(bf_group *g, int i);
int bf_group_set_cameras(bf_group *g, const float *c2w, const float *K);
int bf_group_set_keypoints(bf_group *g, const float *keypoints, const int32_t *n_use_frames);
int bf_group_set_init(bf_group *g, const float *init_betas, const float *init_pose);
/* the whole job's next frames without draining the devices (bf_batch_stage_inputs per device) */
int bf_group_stage_inputs(bf_group *g, const float *keypoints, const int32_t *n_use_frames, const float *init_betas, const float *init_pose);
/* masks[F,M,H,W] + optional contours of the whole job (bf_batch_set_masks per device; the devices extract their contours side by side) */
int bf_group_set_masks(bf_group *g, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks,
                       const int32_t *contour_count, const float *contour_xy, int contour_select);
int bf_group_stage_masks(bf_group *g, int n_masks, const int32_t *view_index, int H, int W, const uint8_t *masks, int contour_select);   /* bf_batch_stage_masks, every device its block */
/* scans[F]: frame f's scan must have been created on the device of f's block (bf_group_shard); NULL detaches */
int bf_group_set_scans(bf_group *g, bf_scan *const *scans);
/* Every device's bf_fit is issued from a host thread of its own (created with the group), so the devices run side by side also
 * when a call enqueues hundreds of launches (silhouette / scan losses); returns when all calls have returned. */
int bf_group_fit(bf_group *g, int n_iters, const bf_hyper *hyper, uint32_t flags);
int bf_group_fit_displacement(bf_group *g, int n_iters, const bf_hyper *hyper);
int bf_group_sync(bf_group *g);
/* ranks of the group's RCCL communicator (created on first use) */
int bf_group_comm_size(bf_group *g);
/* the path's one collective: grouped ncclAllGather of the packed parameters, stream-ordered behind the fits;
 * params[F][n_params] (host) = the copy that arrived on device `from_peer` */
int bf_group_gather_params(bf_group *g, float *params, int from_peer);

/* One process PER device (launched like `torch.distributed.run`: RANK / LOCAL_RANK / WORLD_SIZE in the environment):
 * rank 0 calls bf_comm_unique_id and hands the 128 bytes to the other ranks through the host (bodyfitting_amd/shard.py
 * uses the file system), every rank calls bf_comm_create (ncclCommInitRank). */
typedef struct bf_comm bf_comm;
int bf_comm_unique_id(uint8_t id[128]);
int bf_comm_create(const uint8_t id[128], int rank, int world, int device, bf_comm **out);
void bf_comm_destroy(bf_comm *c);
int bf_comm_size(const bf_comm *c);
int bf_comm_barrier(bf_comm *c);                              /* device idle + every rank arrived */
int bf_comm_allreduce(bf_comm *c, double *value, int op);    /* in place over the ranks; op 0 = sum, 1 = max */
/* the batch holds block `rank` of bf_shard_range(n_frames, world, .); params[n_frames][n_params] (host) on every rank */
int bf_comm_gather_params(bf_comm *c, bf_batch *b, int n_frames, float *params);

/* ---- texture fitting (smplify/texture_fitting.py:220-301) -------------------------------------------------------
 * The loop of TextureFitting.__call__ (:240-275): per iteration both meshes are rendered from one view with neural_renderer
 * (Renderer.render_rgb, camera_mode='projection', ambient light only, anti-aliasing by 2 x 2 super-sampling), the loss is
 * sum |scan_img - smpl_img| and Adam steps the per-face texture cubes of the SMPL+D mesh; only the textures are differentiated.
 * The rasteriser, texture sampling and backward_textures of thirdparty/neural_renderer (cuda/rasterize_cuda_kernel.cu:24-252,
 * 498-540) are restated as HIP kernels; the UV-space texture image of :298 is bf_texfit_render_ndc; the texture cubes of
 * nr.load_obj are bf_texfit_load_textures (the OBJ / MTL / image files are read by bodyfitting_amd/obj_textures.py); the inpainting
 * CNN and the cv2 morphology of render_texture_map's `morph` branch are out of scope. */
typedef struct bf_texfit bf_texfit;
int bf_texfit_create(int device, int image_size, int texture_size, float near, float far, const float *background /*[3] or NULL = white*/,
                     int anti_aliasing, bf_texfit **out);
void bf_texfit_destroy(bf_texfit *x);
/* which: 0 = target (textured scan), 1 = the mesh whose textures are fitted; textures[n_faces][ts][ts][ts][3] */
int bf_texfit_set_mesh(bf_texfit *x, int which, int n_verts, const float *verts, int n_faces, const int32_t *faces, const float *textures);
/* Renderer.render_rgb: R[9], t[3] (world to camera), K[9], orig_size -> rgb[3][image_size][image_size] */
int bf_texfit_render(bf_texfit *x, int which, const float *R, const float *t, const float *K, float orig_size, float *rgb);
/* Renderer.render_texture (thirdparty/neural_renderer/neural_renderer/renderer.py:294-346), the rasteriser behind render_texture_map
 * (smplify/texture_fitting.py:149-151) and the UV-space texture image smpl.png (:298): a mesh whose vertices ndc[n_verts][3] are
 * ALREADY normalised device coordinates (the OBJ's vt lines mapped to [-1, 1], z = 1; the caller appends the reversed faces with
 * their cube axes swapped, renderer.py:338-340) is rasterised without projection -> rgb[3][image_size][image_size],
 * depth[image_size][image_size] (far where nothing was drawn); either may be NULL. */
int bf_texfit_render_ndc(bf_texfit *x, int n_verts, const float *ndc, int n_faces, const int32_t *faces, const float *textures, float *rgb, float *depth);
/* Renderer.render (renderer.py:234-292, nr.rasterize_rgbad) as utils/renderer.py:50-55 calls it: bf_texfit_render's rgb, plus
 * depth[image_size][image_size], flipped and 2 x 2-pooled like the colours (far where nothing was drawn); either may be NULL. */
int bf_texfit_render_depth(bf_texfit *x, int which, const float *R, const float *t, const float *K, float orig_size, float *rgb, float *depth);
/* nr.load_obj(..., load_texture=True)'s texture cubes (neural_renderer/load_obj.py:31-95, cuda/load_textures_cuda_kernel.cu) in one
 * launch over every face: face_uv[n_faces][3][2] (the faces' `vt` corners), face_image[n_faces] (index into images, -1 = none: the
 * face gets face_fill[n_faces][3], the 0.5 default or its material's Kd), images[j] = the decoded file, uint8 [heights[j]][widths[j]][3]
 * top row first (the vertical flip and / 255 happen on the device), wrapping 0 REPEAT / 1 MIRRORED_REPEAT / 2 CLAMP_TO_EDGE /
 * 3 CLAMP_TO_BORDER, bilinear 0 / 1 -> textures[n_faces][ts][ts][ts][3] (host).  Wrapping is applied once per face (DESIGN.md
 * section 2).  texture_size in [2, 256].  ms (may be NULL) receives the upload, kernel and download times from HIP events. */
int bf_texfit_load_textures(int device, int n_faces, const float *face_uv, const int32_t *face_image, const float *face_fill, int n_images,
                            const uint8_t *const *images, const int32_t *heights, const int32_t *widths, int texture_size, int wrapping,
                            int bilinear, float *textures, float *ms /*[3]*/);
/* one iteration (:262-270) from this view; *loss (may be NULL) = the loss before the step */
int bf_texfit_step(bf_texfit *x, const float *R, const float *t, const float *K, float orig_size, float lr, double *loss);
/* loss and d loss / d textures [n_faces][ts][ts][ts][3] of the fitted mesh from this view, without a step */
int bf_texfit_loss_grad(bf_texfit *x, const float *R, const float *t, const float *K, float orig_size, double *loss, float *grad);
int bf_texfit_get_textures(bf_texfit *x, float *textures);

/* ---- neural_renderer.Renderer, stand-alone (thirdparty/neural_renderer/neural_renderer/renderer.py:11-346) --------------------------
 * The renderer of the torch loop of smplify/texture_fitting.py:240-275 and of utils/io_utils.py's lit renders as an object of its
 * own, camera_mode='projection' with zero distortion: a renderer (image size, planes, background, light), meshes resident on its
 * device, and per render a tape from which the textures' gradient of ANY rgb cotangent is formed (backward_textures,
 * cuda/rasterize_cuda_kernel.cu:498-540).  bodyfitting_amd/neural_renderer.py is the drop-in `import neural_renderer` on top.
 * Limits: image_size in [1, 4096], texture_size 0 (a mesh without textures) or in [2, 16], 2 x n_faces inside an int -
 * BF_ERR_UNSUPPORTED above the upper ends; inconsistent arguments are BF_ERR_INVALID before any launch. */
typedef struct bf_nr bf_nr;
typedef struct bf_nr_mesh bf_nr_mesh;
typedef struct bf_nr_tape bf_nr_tape;
/* Renderer.__init__ (renderer.py:12-63): anti_aliasing = 2 x 2 super-sampling, background[3] (NULL: black, the reference's default),
 * near < far.  The light starts as the reference's defaults (:17-19): ambient 0.5, directional 0.5, white, direction (0, 1, 0). */
int bf_nr_create(int device, int image_size, int anti_aliasing, float near, float far, const float *background, bf_nr **out);
void bf_nr_destroy(bf_nr *r);
/* light_intensity_ambient / _directional, light_color_ambient[3] / _directional[3], light_direction[3] (renderer.py:55-60) as
 * nr.lighting (lighting.py:5-57) reads them; a term whose intensity is exactly 0 is skipped (:36,40) */
int bf_nr_set_light(bf_nr *r, float ambient, float directional, const float *color_ambient, const float *color_directional, const float *direction);
/* the `vertices`, `faces`, `textures` arguments of Renderer.render* (renderer.py:65-292) kept on the renderer's device:
 * verts[n_verts][3], faces[n_faces][3] (an index outside [0, n_verts): BF_ERR_INVALID), textures[n_faces][ts][ts][ts][3] or NULL
 * (set them later; texture_size 0 with NULL: a mesh for silhouette / depth renders only) */
int bf_nr_mesh_create(bf_nr *r, int n_verts, const float *verts, int n_faces, const int32_t *faces, int texture_size, const float *textures,
                      bf_nr_mesh **out);
/* new texture values for the same mesh (texture_fitting.py:270: what optimizer.step() changed); tapes made before stay valid */
int bf_nr_mesh_set_textures(bf_nr_mesh *m, const float *textures);
void bf_nr_mesh_destroy(bf_nr_mesh *m);
/* Renderer.render / render_rgb / render_silhouettes / render_depth (renderer.py:82-292) and, with ndc != 0, render_texture's
 * rasterisation (:334-346: the vertices are normalised device coordinates already; K, R, t, orig_size are ignored).  K[9], R[9], t[3]
 * world to camera (projection.py:6-42).  fill_back (:176-178): every face is also drawn with its corners reversed and its texture
 * cube's axes 0 and 2 exchanged - without a doubled texture copy.  lightoff (:180): no lighting; otherwise every face record is lit
 * from its world-space corners (lighting.py:5-57).  -> rgb[3][image_size][image_size], depth[image_size][image_size] (far where
 * empty) and alpha[image_size][image_size] (rasterize.py:181-184), flipped and 2 x 2-pooled (rasterize.py:305-326); each may be NULL.
 * tape (may be NULL) receives what bf_nr_tape_texture_grad needs of THIS render.  rgb or a tape of a mesh without textures, a mesh
 * of another renderer: BF_ERR_INVALID.  Tile lists that overflow their first guess are grown and the render repeated. */
int bf_nr_render(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                 float *rgb, float *depth, float *alpha, bf_nr_tape **tape);
/* backward_textures (cuda/rasterize_cuda_kernel.cu:498-540) of the taped render through pooling, flip, background mask, sampling
 * weight x light and the back records' axis exchange: grad_rgb[3][image_size][image_size] ->
 * grad_textures[n_faces][ts][ts][ts][3], fully written (front and back contributions of a face add).  The textures themselves are
 * not read: the tape outlives bf_nr_mesh_set_textures and its mesh.  A tape whose renderer was destroyed: BF_ERR_INVALID. */
int bf_nr_tape_texture_grad(bf_nr_tape *tape, const float *grad_rgb, float *grad_textures);
/* new positions verts[n_verts][3] for the same topology (what optimizer.step() changed); tapes made before stay valid */
int bf_nr_mesh_set_vertices(bf_nr_mesh *m, const float *verts);
/* bf_nr_render with a say in what the tape keeps: tape_flags is a non-empty set of the two below (bf_nr_render with a tape is
 * BF_NR_TAPE_TEXTURES).  A geometry tape owns, beside a texture tape's pixel map, face records and light rows: this render's
 * vertices (world and projected), K, R, t, orig_size, the light, the super-sampled colours with the background and - lit, with a
 * directional term - the unlit texture sample per pixel; it shares the mesh's faces and vertex -> (record, corner) table by
 * reference count.  It outlives bf_nr_mesh_set_textures, bf_nr_mesh_set_vertices and its mesh.  Without BF_NR_TAPE_TEXTURES (and
 * without rgb) the mesh needs no textures. */
#define BF_NR_TAPE_TEXTURES 1
#define BF_NR_TAPE_GEOMETRY 2
int bf_nr_render_taped(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                       float *rgb, float *depth, float *alpha, int tape_flags, bf_nr_tape **tape);
/* backward_pixel_map and backward_depth_map (cuda/rasterize_cuda_kernel.cu:245-503,543-592) of the taped render for the cotangents
 * of its outputs (each in its output's shape, NULL = zero), the reverse of the light (lighting.py:41-52) for a lit colour render, the
 * sum over each vertex's face corners and the reverse of projection.py:19-42 -> grad_verts[n_verts][3], fully written, and
 * grad_R[9], grad_t[3] (each may be NULL).  After an ndc render grad_verts is with respect to the vertices as given and grad_R /
 * grad_t must be NULL.  K is not differentiated.  A line of an edge that is axis-parallel at an integer pixel coordinate (0 / 0 in
 * the reference) is skipped.  Equal inputs give equal bits.  BF_ERR_INVALID: a tape without BF_NR_TAPE_GEOMETRY, a cotangent for an
 * output the render did not produce, a tape whose renderer was destroyed. */
int bf_nr_tape_vertex_grad(bf_nr_tape *tape, const float *grad_rgb, const float *grad_depth, const float *grad_alpha, float *grad_verts, float *grad_R,
                           float *grad_t);
void bf_nr_tape_destroy(bf_nr_tape *tape);

/* The device route of the three calls above (see bf_workspace): the caller's arrays are read and written where they lie, on
 * `stream`, and nothing is copied through the host.  Each counts as a *_dev call in bf_dev_route_stats; bf_nr_render[_taped],
 * bf_nr_tape_texture_grad and bf_nr_tape_vertex_grad count as host calls.  One workspace per renderer.
 *
 * bf_nr_render_dev: bf_nr_render_taped's arguments, then verts[n_verts][3] and textures[n_faces][ts][ts][ts][3] of THIS render
 * as device pointers (the mesh supplies the topology, the texture size and its tile lists; what bf_nr_mesh_create or
 * bf_nr_mesh_set_* uploaded is not read), rgb / depth / alpha device pointers, and the camera: each of K, R, t EITHER as the host
 * pointer of bf_nr_render_taped (taken by value) OR as a device pointer in `cam` (taken by address, never read back) - `cam` NULL
 * or a NULL member: by value.  A tape borrows its storage: tape_storage, a float32 device array of at least the total
 * bf_nr_tape_layout gives for this render (tape_floats says how many it holds), which must stay alive and unwritten until the last
 * gradient call of the tape has run on the device; such a tape owns no device memory, bf_nr_tape_destroy of it waits for nothing,
 * and it takes the *_dev gradient calls only.  Without a tape, tape_storage is not read.
 * The call returns when its work is queued, with ONE wait inside: the tile lists' total (4 bytes) is read back behind the
 * projection, the count pass and the scan, through an event recorded there - not the stream's later work - so that lists that
 * are too short are grown BEFORE the fill pass: a render is never repeated and no output is written from a truncated list.
 * Neither gradient call waits for anything.  Refusals: the host twins', and BF_ERR_INVALID for no workspace or one of another
 * device, a NULL vertex pointer, K / R / t given both ways, tape storage that is NULL or too small when a tape is asked for. */
typedef struct bf_nr_camera_dev { const float *K, *R, *t; } bf_nr_camera_dev;
int bf_nr_render_dev(bf_nr *r, bf_nr_mesh *m, const float *K, const float *R, const float *t, float orig_size, int fill_back, int lightoff, int ndc,
                     float *rgb, float *depth, float *alpha, int tape_flags, bf_nr_tape **tape, const float *verts, const float *textures,
                     const bf_nr_camera_dev *cam, float *tape_storage, size_t tape_floats, bf_workspace *ws, void *stream);
/* cotangents and gradients as device pointers; grad_textures is fully written, grad_verts too, grad_R[9] / grad_t[3] where given */
int bf_nr_tape_texture_grad_dev(bf_nr_tape *tape, const float *grad_rgb, float *grad_textures, bf_workspace *ws, void *stream);
int bf_nr_tape_vertex_grad_dev(bf_nr_tape *tape, const float *grad_rgb, const float *grad_depth, const float *grad_alpha, float *grad_verts, float *grad_R,
                               float *grad_t, bf_workspace *ws, void *stream);
/* where a tape's buffers lie in its storage (csrc/nr_tape_layout.h), in floats: out[0..7] the offsets (multiples of 64) and
 * out[8..15] the sizes (0: absent) of view | pixel map | face records | light rows | vertices | projected vertices | colour map |
 * unlit samples, out[16] the total.  is: the super-sampled size, nrec: n_faces or 2 n_faces (fill_back), lit: the render is lit,
 * flags: BF_NR_TAPE_* (0: a render without a tape), has_rgb: it makes rgb, directional: the light's directional term is not 0. */
int bf_nr_tape_layout(int is, int nrec, int nv, int lit, int flags, int has_rgb, int directional, uint64_t out[17]);
/* test hook, process-wide: out[0] renders of bf_nr_render_dev, out[1] tile lists it grew, out[2] bytes read back to the host by
 * the device-route calls */
int bf_nr_route_stats(int64_t out[3]);

/* ---- HMR initial estimate (smplify/body_fitting.py:17-75, models/hmr.py) ----------------------------------------------------------
 * The reference's run_hmr on the GPU in fp32: cv2.resize to 224 x 224 (INTER_LINEAR, OpenCV's 8-bit fixed-point arithmetic), /255,
 * Normalize(IMG_NORM_MEAN, IMG_NORM_STD), ResNet-50 v1.5 in eval() and the iterative regressor (n_iter = 3).  Weights are packed by
 * bodyfitting_amd/hmr.py in the order hmr_api.hip lists them, BatchNorm folded into each convolution (bf_hmr_n_weights floats);
 * mean_params[157] = init_pose[144] | init_shape[10] | init_cam[3].  images[n][H][W][3] uint8 RGB, 1 <= n <= max_batch.
 * rot6d_to_rotmat, the caller's root rotation and the rotation-matrix -> axis-angle conversion run on the host (hmr.py). */
typedef struct bf_hmr bf_hmr;
int64_t bf_hmr_n_weights(void);
int bf_hmr_create(int device, const float *weights, int64_t n_weights, const float *mean_params, int max_batch, bf_hmr **out);
void bf_hmr_destroy(bf_hmr *h);
/* the regressor's final state: pose6d[n][144] (24 x the 6D rotation), betas[n][10], cam[n][3] */
int bf_hmr_predict(bf_hmr *h, int n, int H, int W, const uint8_t *images, float *pose6d, float *betas, float *cam);
/* the pooled backbone features xf[n][2048] */
int bf_hmr_features(bf_hmr *h, int n, int H, int W, const uint8_t *images, float *xf);
/* the image pipeline alone: resized[n][224][224][3] uint8 and / or normalized[n][224][224][3] fp32 (either may be NULL) */
int bf_hmr_preprocess(bf_hmr *h, int n, int H, int W, const uint8_t *images, uint8_t *resized, float *normalized);
/* test hook: one convolution of the HMR kernel on host arrays - x[n][H][W][cin] NHWC, w[k*k*cin][cout] in (ky, kx, ci) order,
 * bias[cout], res[n][Ho][Wo][cout] or NULL, relu 0/1 -> y[n][Ho][Wo][cout] */
int bf_hmr_selftest_conv(int device, int n, int H, int W, int cin, int cout, int k, int stride, int pad, const float *x, const float *w,
                         const float *bias, const float *res, int relu, float *y);

/* ---- OpenPose body estimator (openpose/body.py Body.__call__, openpose/model.py bodypose_model) -------------------------------------
 * The COCO-18 body CPM on the GPU in fp32 at body.py's four scales: cv2.resize INTER_CUBIC (OpenCV's 11-bit fixed-point path),
 * padRightDownCorner, /256 - 0.5, the VGG front and six two-branch stages; then per scale the float cubic x8 resize, the crop and the
 * cubic resize to the original, accumulated into float64 heatmap_avg[n][H][W][19] / paf_avg[n][H][W][38] in body.py's operation
 * order (heatmap_avg += heatmap_avg + heatmap / 4).  Weights are packed by bodyfitting_amd/openpose.py in the order openpose_api.hip
 * lists them (bf_openpose_n_weights floats).  bgr[n][H][W][3] uint8, 1 <= n <= max_batch, 13 <= H <= max_h, 13 <= W <= max_w; one
 * call takes images of one size.  Each maps / inject call leaves its maps resident for bf_openpose_peaks and bf_openpose_pairs; the
 * greedy connection pick and the subset assembly run on the host (openpose.py). */
typedef struct bf_openpose bf_openpose;
int64_t bf_openpose_n_weights(void);
int bf_openpose_create(int device, const float *weights, int64_t n_weights, int max_batch, int max_h, int max_w, bf_openpose **out);
void bf_openpose_destroy(bf_openpose *op);
/* the accumulated maps; heat / paf may be NULL (the maps stay resident either way) */
int bf_openpose_maps(bf_openpose *op, int n, int H, int W, const uint8_t *bgr, double *heat, double *paf);
/* the network alone: per scale (0.5, 1, 1.5, 2 x 368 / H), concatenated, inputs[n][Hp][Wp][4] (channel 3 zero; may be NULL) and
 * outputs[n][Hp/8][Wp/8][57] (Mconv7_stage6_L1 0:38, Mconv7_stage6_L2 38:57) */
int bf_openpose_network(bf_openpose *op, int n, int H, int W, const uint8_t *bgr, float *inputs, float *outputs);
/* test hook: everything after the network on injected per-scale outputs (bf_openpose_network's layout, n_outputs floats) */
int bf_openpose_inject(bf_openpose *op, int n, int H, int W, const float *outputs, int64_t n_outputs, double *heat, double *paf);
/* hw[2] = (H, W) of the resident maps */
int bf_openpose_map_size(bf_openpose *op, int *hw);
/* on the resident maps of the first n views: gaussian_filter(sigma=3) of parts 0..17 (blurred[n][H][W][18], may be NULL) and the
 * peaks (> 0.1 and >= the four neighbours): counts[n], peaks[n][cap][3] = (x, y, part), scores[n][cap] = heatmap_avg there, in no
 * particular order.  More than cap peaks in a view: BF_ERR_UNSUPPORTED. */
int bf_openpose_peaks(bf_openpose *op, int n, int cap, double *blurred, int *counts, int *peaks, double *scores);
/* limb scores on the resident paf_avg of one view: jobs[npairs][5] = (limb 0..18, ax, ay, bx, by) -> score[npairs]
 * (score_with_dist_prior) and above[npairs] (samples of the 100 > 0.05) */
int bf_openpose_pairs(bf_openpose *op, int view, int npairs, const int *jobs, double *score, int *above);
/* test hook: one convolution of the OpenPose kernel (stride 1, padding k / 2, k = 1, 3 or 7) on host arrays - x[n][H][W][cin],
 * w[k*k*cin][cout] in (ky, kx, ci) order, bias[cout], relu 0/1 -> y[n][H][W][cout] */
int bf_openpose_selftest_conv(int device, int n, int H, int W, int cin, int cout, int k, int relu, const float *x, const float *w,
                              const float *bias, float *y);

/* ---- OpenPose hand estimator (openpose/hand.py Hand.__call__, openpose/model.py handpose_model, openpose/util.py npmax) -------------
 * The 21-part hand CPM on crops of views, in fp32 at hand.py's four scales, through the body estimator's convolution kernels: per crop
 * cv2.resize INTER_CUBIC (uint8, the crop's own edges replicated), padRightDownCorner, /256 - 0.5, the VGG front and five stages; then
 * the float x8 resize, the crop and the resize to the crop's size, accumulated into float64 heatmap_avg (+= heatmap / 4).  Crops of
 * one network size run as one batch (up to max_hands).  Weights are packed by bodyfitting_amd/openpose_hand.py in the order
 * openpose_hand_api.hip lists them (bf_openpose_hand_n_weights floats).  bgr[n_views][H][W][3] uint8, 13 <= H <= max_h,
 * 13 <= W <= max_w; boxes[n_hands][5] = (view, x, y, w, h), the crop bgr[view][y:y+h, x:x+w], inside its view and at least 13 on a
 * side (anything else: BF_ERR_INVALID).  Each maps / inject call leaves its maps resident for bf_openpose_hand_peaks. */
typedef struct bf_openpose_hand bf_openpose_hand;
int64_t bf_openpose_hand_n_weights(void);
int bf_openpose_hand_create(int device, const float *weights, int64_t n_weights, int max_hands, int max_h, int max_w, bf_openpose_hand **out);
void bf_openpose_hand_destroy(bf_openpose_hand *h);
/* heat: per crop heatmap_avg[h][w][22] float64, the crops end to end in box order (may be NULL) */
int bf_openpose_hand_maps(bf_openpose_hand *h, int n_views, int H, int W, const uint8_t *bgr, int n_hands, const int *boxes, double *heat);
/* the network alone: per scale (0.5, 1, 1.5, 2 x 368 / h), per crop in box order, concatenated, inputs[Hp][Wp][4] (channel 3 zero;
 * may be NULL) and outputs[Hp/8][Wp/8][22] (Mconv7_stage6) */
int bf_openpose_hand_network(bf_openpose_hand *h, int n_views, int H, int W, const uint8_t *bgr, int n_hands, const int *boxes, float *inputs,
                             float *outputs);
/* test hook: everything after the network on injected outputs (bf_openpose_hand_network's layout, n_outputs floats); only the boxes'
 * w and h are read */
int bf_openpose_hand_inject(bf_openpose_hand *h, int n_hands, const int *boxes, const float *outputs, int64_t n_outputs, double *heat);
/* on the n resident crops (n = the last call's n_hands), per part 0..20: gaussian_filter(sigma=3) (blurred: per crop [h][w][21] end to
 * end, may be NULL); the 8-connected components of blurred > 0.05, the one with the largest np.sum of heatmap_avg (the first on a
 * tie), and util.npmax of heatmap_avg zeroed off it -> peaks[n][21][2] = (x, y) in crop coordinates, scores[n][21] = the zeroed map
 * there, found[n][21] = 1; an empty mask gives (0, 0), 0, 0 */
int bf_openpose_hand_peaks(bf_openpose_hand *h, int n, double *blurred, int *peaks, double *scores, int *found);
/* test hook: skimage.measure.label(binary, connectivity=2) of binary[n][H][W] (0 / 1) -> labels[n][H][W] (0 off the mask, components
 * numbered 1.. by the raster order of their first pixel), counts[n] */
int bf_openpose_hand_selftest_label(int device, int n, int H, int W, const uint8_t *binary, int *labels, int *counts);

/* ---- GeneBody view preparation (apps/genebody_fitting.py:111-142 get_data, utils/io_utils.py:97-136 image_cropping) ----------------
 * Every view of a frame at once.  bf_views_bbox uploads the masks whole (masks[n] -> [H][W] uint8 each, one size per call) and leaves
 * them resident: bbox[n][4] = (top, left, bottom, right), the min / max row and column of mask != 0 (max inclusive, as np.max of
 * np.where); a view whose mask is empty is an error that names it.  The crop rectangle is image_cropping's host arithmetic
 * (bodyfitting_amd/genebody.py); bf_views_prepare takes the rectangle numpy slicing reads, rects[n][4] = (top, left, bottom, right)
 * with 0 <= top < bottom <= H and 0 <= left < right <= W, uploads only the rows top..bottom of each images[i] ([H][W][3] uint8, RGB), per
 * view, writes cv2.resize((img * (msk > 128)[..., None])[top:bottom, left:right], (L, L)) to out_images[n][L][L][3], the mask crop
 * resized the same way to out_masks[i] ([n][L][L]; only where mask_view[i] != 0), and sums[i] = the integer sum of view i's
 * resized bytes (np.mean(img) > 10 <=> sums[i] > 30 L^2).  Both resizes are INTER_LINEAR in OpenCV's 8-bit fixed-point arithmetic
 * (the app passes its INTER_CUBIC / INTER_NEAREST as the positional dst).  Buffers start at the sizes given to create and grow. */
typedef struct bf_views bf_views;
int bf_views_create(int device, int max_views, int max_h, int max_w, int L, bf_views **out);
void bf_views_destroy(bf_views *v);
int bf_views_bbox(bf_views *v, int n, int H, int W, const uint8_t *const *masks, int *bbox);
int bf_views_prepare(bf_views *v, int n, const int *rects, const uint8_t *const *images, const int *mask_view, uint8_t *out_images,
                     uint8_t *out_masks, int64_t *sums);
/* device time of the last calls from HIP events on the object's stream: ms[6] = bbox (mask upload, kernels, download), prepare (crop
 * upload, kernel, download); bytes[3] = masks up, crops (+ job table) up, results down */
int bf_views_last_timing(bf_views *v, float *ms, int64_t *bytes);

/* ---- LBAM texture inpainting (models/inpaint.py Inpainter, LBAMModel(4, 3); smplify/texture_fitting.py:191-214 inpaint) ------------
 * The network in fp32 on the exact-fp32 MFMA, NHWC.  Weights are packed by bodyfitting_amd/inpaint.py in the order inpaint_api.hip
 * lists them (bf_inpaint_n_weights floats, the clamped GaussActivation parameters last).  Images are uint8 [n][H][W][3]; H and W are
 * multiples of 128 within max_h x max_w and 1 <= n <= max_batch (anything else: BF_ERR_INVALID).  face_uv[n_faces][3][2] float32 are
 * the UV triangles in pixels (load_obj_uv(...) * H). */
typedef struct bf_inpaint bf_inpaint;
int64_t bf_inpaint_n_weights(void);
int bf_inpaint_create(int device, const float *weights, int64_t n_weights, int max_batch, int max_h, int max_w, bf_inpaint **out);
void bf_inpaint_destroy(bf_inpaint *h);
/* Inpainter.__call__ per image: mask 255 = hole (a byte >= 128 counts); out[n][H][W][3] float32, known pixels float32(v / 255) */
int bf_inpaint_run(bf_inpaint *h, int n, int H, int W, const uint8_t *image, const uint8_t *mask, float *out);
/* the hole mask of TextureFitting.inpaint: the faces with more than 63 / 6 grey samples, filled as cv2.drawContours(..., -1) fills
 * them -> mask[H][W][3] (0 / 255); a sample index outside [-size, size) (numpy's IndexError) is BF_ERR_INVALID */
int bf_inpaint_hole_mask(bf_inpaint *h, int H, int W, const uint8_t *img, int n_faces, const float *face_uv, uint8_t *mask);
/* the whole of TextureFitting.inpaint on img[H][W][3] -> out[H][W][3]; mask (may be NULL) receives the hole mask */
int bf_inpaint_texture(bf_inpaint *h, int H, int W, const uint8_t *img, int n_faces, const float *face_uv, uint8_t *out, uint8_t *mask);
/* cv2.erode (op 0) / cv2.dilate (op 1) with np.ones((k, k)) (odd k <= 31), pixels outside the image ignored, on in[n][H][W][C] */
int bf_morph_u8(int device, int op, int k, int n, int H, int W, int C, const uint8_t *in, uint8_t *out);
/* test hook: the face test alone -> selected[n_faces] (0 / 1) */
int bf_inpaint_select_faces(bf_inpaint *h, int H, int W, const uint8_t *img, int n_faces, const float *face_uv, uint8_t *selected);
/* test hook: one convolution of the inpainting kernels on host arrays, no epilogue - deconv 0: 4 x 4, stride 2, padding 1 of
 * x[n][H][W][cin] (cin a multiple of 4) with w packed [16 cin][coutp] in (ky, kx, ci) order -> y[n][H/2][W/2][cout], and with xm / wm
 * (may be NULL) the second operand of the same launch -> ym; deconv 1: ConvTranspose2d(4, 2, 1) with w packed per phase
 * [4][4 cin][coutp] -> y[n][2H][2W][cout].  coutp = cout rounded up to 4. */
int bf_inpaint_selftest_conv(int device, int deconv, int n, int H, int W, int cin, int cout, const float *x, const float *xm, const float *w,
                             const float *wm, float *y, float *ym);

/* ---- fit-check overlay (smplify/body_fitting.py:34-42 check_smpl_fitting) -------------------------------------------------------
 * n views at once: images[n] -> [H][W][3] uint8 each, verts[nv][3] float32, cams[n][21] double = the rotation R'[3][3] (row-major)
 * cv2.projectPoints rebuilds from the Rodrigues vector, t[3] and K[3][3].  Every vertex is projected as cv2.projectPoints does with
 * zero distortion (double, rounded to float32); one with 0 <= x < W and 0 <= y < H is truncated to (int x, int y) and stamped as
 * cv2.circle(img, (x, y), 1, (0, 255, 0), -1) draws it (the plus of five pixels, clipped at the edges) -> out[n][H][W][3] */
int bf_overlay_stamp(int device, int n, int H, int W, const uint8_t *const *images, int nv, const float *verts, const double *cams,
                     uint8_t *out);

/* Device time of the kernels of the last bf_fit on this batch, from HIP events on the batch's
 * stream: ms[0] = fit loop kernel(s), ms[1] = final full-mesh forward kernel, ms[2] = joints kernel +
 * result fetch, ms[3] = whole call.  (With BF_FIT_DENSE every iteration's mesh pass is inside ms[0].) */
int bf_batch_last_timing(bf_batch *b, float ms[4]);
/* The same, summed over every bf_fit since bf_batch_timing_reset (at most 1024 calls are kept);
 * *n_calls receives how many were summed. */
int bf_batch_timing_reset(bf_batch *b);
int bf_batch_timing_sum(bf_batch *b, float ms[4], int32_t *n_calls);
/* Duration of the single-frame full-mesh forward (bf_mesh_kernel, the HBM-bound kernel of the keypoint-only path) measured INSIDE the
 * kernel: first workgroup's start to last workgroup's end on the device's 100 MHz clock, `reps` launches on frame 0's current pose state;
 * us[3] = mean, min, max in microseconds.  What bench.py's roofline_mesh divides the kernel's algorithmic bytes by (an event bracket
 * around a 6 us kernel is half record overhead).  SMPL-sized models. */
int bf_batch_mesh_span(bf_batch *b, int reps, float us[3]);
/* Device time of the kernel classes of the LAST dense iteration (smplify.py:177-213 with use_mask / use_mesh / SMPL-X keypoints) of the
 * last bf_fit, from HIP events on the batch's stream: ms[0] pose state + forward mesh pass, ms[1] keypoint loss and / or silhouette kernels,
 * ms[2] closest-point search, ms[3] point-cloud loss + gradient, ms[4] reverse mesh pass, ms[5] reduction of the partial blocks.  `enable`
 * switches the recording for the following fits (the events cost a few microseconds of that one iteration); ms may be NULL. */
int bf_batch_dense_timing(bf_batch *b, int enable, float ms[6]);
/* How the dense iterations of this batch's fits have run: 1 = with the fit kernel resident (one launch per fit on its own stream, paced by
 * doorbells), 0 = one fit launch per iteration (the self-test found the two streams on one hardware queue - libbodyfit says so once on
 * stderr - or BF_DENSE_PERSISTENT=0, or 16+ frames), -1 = no dense fit has run yet.  Same results either way; ~3x the time without. */
int bf_batch_dense_resident(const bf_batch *b);

/* ---- test hooks (bring-up / parity tests only; not part of the drop-in surface) ----------------------------------
 * first-iteration intermediates of frame 0 written by the last bf_loss_grad launch (layout: tests/gpu_debug.py) */
int bf_batch_debug_dump(bf_batch *b, float *dst, int n);
/* first Adam moment of the SMPL+D displacement (after one step = 0.1 x the gradient) */
int bf_batch_debug_disp_moment(bf_batch *b, float *m_out);
/* second Adam moment of the SMPL+D displacement, [F,NV,3] like the first */
int bf_batch_debug_disp_moment2(bf_batch *b, float *v_out);
/* vertices[F,NV,3]: the body vertices the last full-model mesh pass of the batch left on the device (after bf_dense_iter_grad
 * without BF_DENSE_GRAD_SUBMODEL: the ones its losses were evaluated at) */
int bf_batch_debug_vertices(bf_batch *b, float *vertices);
/* Fit-lane groups of the batch since it was created (lanes.hip; BF_FIT_LANES, BF_FIT_LANE_WIDTH): out[0] lane launches, out[1] the
 * frame-after-frame calls they carried, out[2] the most calls one launch carried, out[3] W, the most it may carry (1 without lanes) */
int bf_batch_lane_stats(bf_batch *b, int32_t out[4]);
/* How the fit lanes of the batch were fed since it was created: out[0] input transfers issued (host-fed groups: one per lane launch, and
 * one for a slot that a drain found staged with no call joined; a launch per call, BF_FIT_LANE_WIDTH=1: one per staging), out[1] calls
 * without a staging of their own whose inputs were copied on the host, pinned slot to pinned slot, out[2] such calls whose inputs were
 * copied on the device, out[3] times the host had to wait for a pinned arena's previous transfer before filling it again */
int bf_batch_lane_feed_stats(bf_batch *b, int64_t out[4]);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BODYFIT_H */
