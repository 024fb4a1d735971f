// orbx_kernels.h -- launch interface of the extraction kernels (orbx_extract.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "orbx.h"
#include "orbx_geometry.h"
#include "orbx_match_types.h"

namespace orbx {

// Device-resident buffers for one extractor configuration and batch capacity.
struct DeviceBuffers {
    int batch_cap = 0;
    LevelGeom* lv = nullptr;         // [L]
    CellGeom* cells = nullptr;       // [ncells]
    int16_t* rtab = nullptr;         // resize tables
    uint8_t* pyr = nullptr;          // [B][pyr_frame_bytes] image pyramid (level ROIs)
    uint8_t* blur = nullptr;         // [B][pyr_frame_bytes] Gaussian-blurred levels
    uint8_t* score = nullptr;        // [B][pyr_frame_bytes] FAST strength map M per level
    uint32_t* slots = nullptr;       // [B][slots_per_frame] packed FAST keypoints per cell
    int* cell_count = nullptr;       // [B][ncells]
    uint32_t* keys = nullptr;        // [B][keys_per_frame] packed candidates per level
    int* key_node = nullptr;         // [B][keys_per_frame] octree node of each candidate
    uint32_t* kept = nullptr;        // [B][kept_per_frame] kept keypoints (octree list order)
    int* kept_count = nullptr;       // [B][L]
    uint16_t* dt_list = nullptr;     // [B][kept_per_frame] kept slots listed tile after tile (k_describe_tiles)
    uint32_t* dt_tile = nullptr;     // [B][tiles_total] per level tile: list start << 16 | count
    int* status = nullptr;           // [B] error flags
    unsigned long long* oct_stamps = nullptr;  // [B][L][16] k_octree phase stamps (ORBX_OCT_STAMPS)
};

// Kernel status bits (DeviceBuffers::status)
enum : int { kStatusNodeOverflow = ORBX_STATUS_NODE_OVERFLOW, kStatusIterations = ORBX_STATUS_ITERATIONS };

// The pyramid an extractor kept from its last extraction (mvImagePyramid, ORBextractor.h:162):
// frame f's level l ROI starts at base + f * frame_bytes + off[l], rows pitch[l] bytes apart.
struct PyrView {
    const uint8_t* base = nullptr;
    long long frame_bytes = 0;
    int nframes = 0;           // frames of the last extraction
    int W = 0, H = 0, L = 0;
    long long off[kMaxLevels];
    int pitch[kMaxLevels], w[kMaxLevels], h[kMaxLevels];
    float scale[kMaxLevels], inv_scale[kMaxLevels];
    int device = 0;
    hipStream_t stream = nullptr;  // stream of the last extraction
    // level 0 read in place (orbx_extractor_set_level0_in_place): frame f's level 0 is the
    // caller's frame at l0 + f * l0_fp, rows l0_pitch apart (null: level 0 is in base)
    const uint8_t* l0 = nullptr;
    long long l0_fp = 0;
    int l0_pitch = 0;
};
// Fills `v` for extractor `ex` (ORBX_ERR_STATE before any extraction, and, unless
// allow_l0 -- a reader that takes level 0 from v->l0 --, after an in-place extraction).
int extractor_pyramid(orbx_extractor* ex, PyrView* v, bool allow_l0 = false);

constexpr int kStages = 6;
extern const char* const kStageNames[kStages];

// Pattern + umax into __constant__ memory (idempotent).
hipError_t upload_constants(const OrbParams& prm);

// Enqueue the whole extraction of `batch` device frames on `stream`.
// kps: orbx_keypoint[batch*cap], desc: uint8[batch*cap*32], n_per_frame: int[batch].
// ev (nullable) holds kStages+1 events recorded between the stages.  status_out (nullable,
// e.g. host-mapped memory): the describe kernel copies each frame's octree status word there
// beside its count, so a host call learns both without a separate read-back.
hipError_t launch_extract(const Plan& plan, const DeviceBuffers& db, int batch, const uint8_t* d_imgs,
                          size_t frame_pitch, size_t stride, void* kps, uint8_t* desc, int cap,
                          int* n_per_frame, hipStream_t stream, hipEvent_t* ev,
                          hipEvent_t stage_ev = nullptr, int stage_after = 0, bool l0_in_place = false,
                          int* status_out = nullptr);

// dist[i*nb+j] = Hamming(a_i, b_j)
hipError_t launch_hamming_matrix(const uint8_t* a, int na, const uint8_t* b, int nb, int32_t* dist,
                                 hipStream_t stream);

// The k_proj_search instantiation launch_proj_search chose (diagnostics; host memory):
// query state / descriptors in LDS, the workgroup's threads, its dynamic LDS bytes.
struct ProjForm {
    int qlds, dlds, threads;
    size_t lds;
};

// The form launch_proj_search would run for these sizes: hipErrorInvalidValue where none
// fits the 160 KB of LDS (or max_n >= 8192, noct outside 1..32).  Host arithmetic only, so
// a caller can refuse before its first launch.  split: with split_grids.
hipError_t proj_search_form(int max_n, int max_nq, int noct, bool small, bool tiny, bool lean, bool split,
                            ProjForm* form);

// form (nullable): the form chosen.  Refuses as proj_search_form does, launching nothing.
hipError_t launch_proj_search(const ProjProblem* d_probs, int nprob, const ProjParams& P, unsigned long long* scratch,
                              const long long* d_scratch_off, int max_n, int max_nq, hipStream_t stream,
                              bool small = false, bool tiny = false, bool lean = false,
                              unsigned char* split_grids = nullptr, ProjForm* form = nullptr);

// k_seq_grid + k_seq_score + k_seq_commit: the split form of launch_proj_search for the
// batched sequence matcher (grids: nprob x seq_grid_bytes(cap) bytes of device memory).
// cap: keypoints per problem (the grids); qcap: queries per problem (0: cap).  stage_*
// (one problem only): k_stage_copy first copies stage_bytes (a multiple of 16) from
// device-visible pinned host memory to stage_dst -- the call's inputs, d_probs among them
size_t seq_grid_bytes(int cap, int noct);
// k_stage_copy: bytes (a multiple of 16, 16-byte aligned ends) between device memory and
// device-visible (mapped) pinned host memory, by the GPU's own loads and stores (many
// workgroups) instead of a DMA copy -- for the small per-call copies of the host calls
hipError_t launch_stage_copy(const void* src, void* dst, size_t bytes, hipStream_t stream);
hipError_t launch_seq_split(const ProjProblem* d_probs, int nprob, const ProjParams& P, unsigned char* grids,
                            int cap, unsigned long long* scratch, const long long* d_scratch_off, hipStream_t stream,
                            int qcap = 0, int replay_rt = 0, const void* stage_src = nullptr,
                            void* stage_dst = nullptr, size_t stage_bytes = 0);

hipError_t launch_seq_build(const SeqArgs& A, int npairs, ProjQuery* queries, ProjProblem* probs,
                            long long* scratch_off, hipStream_t stream);
// k_local_build: Tracking::SearchLocalPoints' problem per frame (one workgroup each)
hipError_t launch_local_build(const LocalArgs& A, int batch, ProjQuery* queries, uint8_t* qdesc, ProjProblem* probs,
                              long long* scratch_off, hipStream_t stream);

hipError_t launch_triangulation(const TriProblem* d_probs, int nprob, unsigned long long* scratch, int max_n2,
                                int max_nq, hipStream_t stream);
// k_tri_setup (queries + problems from the keyframe tables) then k_triangulation
hipError_t launch_triangulation_batch(const TriBatch& tb, unsigned long long* scratch, hipStream_t stream);

hipError_t launch_stereo(const StereoBatch& sb, int batch, hipStream_t stream);
// k_stereo_index keeps the (octave, row) counters and the row coverage of one pair in LDS
constexpr size_t kStereoIndexLdsMax = 150 * 1024;
inline size_t stereo_index_lds(int nlevels, int rows) { return ((size_t)nlevels * rows + 1 + rows + 1) * 4; }
hipError_t launch_bow(const BowProblem* d_prob, int n2, int nitems, hipStream_t stream);
hipError_t launch_init(const InitProblem* d_prob, int n1, int n2, int nq, hipStream_t stream);
hipError_t launch_window_best(const BestProblem* d_prob, int nq, hipStream_t stream);
hipError_t launch_distinctive(int nmp, const int32_t* off, const uint8_t* desc, int32_t* best, uint8_t* out_desc,
                              hipStream_t stream);

// k_pose_opt (orbx_poseopt.hip): Optimizer::PoseOptimization for `batch` frames, one workgroup
// each.  Frames of up to kPoseOptLdsEdges edges keep their edge records in LDS (64 KB: two
// workgroups per compute unit), larger ones stream them from the workspace.
constexpr int kPoseOptLdsEdges = ORBX_POSE_OPT_LDS_EDGES;
struct PoseOptArgs {
    const orbx_keypoint* kps;  // [B][cap]
    const int32_t* n;          // [B]
    int cap;
    const float* u_right;      // [B][cap] or null
    int32_t* frame_mp;         // [B][cap]
    const float* pos;          // [n_mp][3]
    int n_mp;
    float inv_sigma2[ORBX_MAX_LEVELS];
    int nlevels;
    float fx, fy, cx, cy, bf;
    float delta_mono, delta_stereo;
    const float* Tcw;          // [B][12]
    float* Tcw_out;            // [B][12]
    uint8_t* outlier;          // [B][cap]
    int32_t* ninliers;         // [B]
    int32_t* ninit;            // [B]
    int32_t* trace;            // [B][4][2] or null
    int discard_outliers;
    const int32_t* mp_obs;     // [n_mp] or null
    int32_t* nmatches_map;     // [B] or null
    float* rec;                // set by launch_pose_opt
    int32_t* eidx;
};
size_t pose_opt_workspace_bytes(int batch, int cap);
hipError_t launch_pose_opt(PoseOptArgs A, int batch, char* workspace, hipStream_t stream);

// k_opt_sim3 (orbx_optsim3.hip): Optimizer::OptimizeSim3 for `batch` loop candidates, one
// workgroup each; the pair records live in the workspace.
struct OptSim3Args {
    int cap1, cap2;
    const int32_t* n1;           // [B]
    const orbx_keypoint* kps1;   // [B][cap1]
    const int32_t* mp1;          // [B][cap1]
    int32_t* matches12;          // [B][cap1] in/out
    const int32_t* idx2;         // [B][cap1]
    const int32_t* n2;           // [B]
    const orbx_keypoint* kps2;   // [B][cap2]
    const float* pos;            // [n_mp][3]
    int n_mp;
    const float* Tcw1;           // [B][12]
    const float* Tcw2;           // [B][12]
    float inv_sigma2_1[ORBX_MAX_LEVELS], inv_sigma2_2[ORBX_MAX_LEVELS];
    int nlevels;
    float K1[4], K2[4];
    const float* R12;            // [B][9]
    const float* t12;            // [B][3]
    const float* s12;            // [B]
    float th2, delta;            // delta: the float sqrt(th2) of Optimizer.cc:1221
    int fix_scale;
    float* R12_opt;              // [B][9]
    float* t12_opt;              // [B][3]
    float* s12_opt;              // [B]
    int32_t* ninliers;           // [B] or null
    int32_t* ncorr;              // [B] or null
    int32_t* nbad;               // [B] or null
    int32_t* trace;              // [B][2][2] or null
    double probes[14 * 8];       // set by launch_opt_sim3: Sim3(+-1e-9 e_d) as q xyzw, t, s
    float* rec;                  // set by launch_opt_sim3
    int32_t* eidx;
    int32_t* active;
};
size_t opt_sim3_workspace_bytes(int batch, int cap1);
hipError_t launch_opt_sim3(OptSim3Args A, int batch, char* workspace, hipStream_t stream);

// k_local_ba (orbx_localba.hip): Optimizer::LocalBundleAdjustment for `batch` local maps, one
// workgroup each; poses, points, edge records, the per-point blocks and the reduced system S
// live in the workspace.
struct LocalBaArgs {
    const int32_t* kf_off;       // [B + 1]
    int n_kf;
    const float* kf_Tcw;         // [n_kf][12]
    const uint8_t* kf_fixed;     // [n_kf]
    const int32_t* kf_slot;      // [n_kf]
    const int32_t* pt_off;       // [B + 1]
    int n_pt;
    const float* pt_pos;         // [n_pt][3]
    const int32_t* obs_off;      // [n_pt + 1]
    int n_obs;
    const int32_t* obs_kf;       // [n_obs]
    const int32_t* obs_kp;       // [n_obs]
    int n_slots, cap;
    const orbx_keypoint* kps;    // [n_slots][cap]
    const float* u_right;        // [n_slots][cap] or null
    float inv_sigma2[ORBX_MAX_LEVELS];
    int nlevels;
    float fx, fy, cx, cy, bf;
    float delta_mono, delta_stereo;
    int max_free;                // free keyframes per problem that S is sized for
    float* kf_Tcw_out;           // [n_kf][12]
    float* pt_pos_out;           // [n_pt][3]
    uint8_t* erase;              // [n_obs]
    uint8_t* level1;             // [n_obs] or null
    int32_t* n_erase;            // [B]
    int32_t* trace;              // [B][2][2] or null
    int32_t* status;             // [B]
    // set by launch_local_ba
    double* pose;                // [n_kf][2][16]: current and trial {q xyzw, t, R row by row}
    double* pt;                  // [n_pt][2][3]: current and trial
    double* pt_sys;              // [n_pt][24]: Hll (6), bl (3), Dinv (9), Dinv bl (3), xl (3)
    double* W;                   // [n_obs][18]: A^T (rho' Omega) B
    double* chi2;                // [n_obs]
    double* S;                   // [B][(6 max_free)^2]
    float* rec;                  // [n_obs][4]: u, v, u_right, invSigma2
    int32_t* rec_kf;             // [n_obs] keyframe row, -1: not an edge
    int32_t* rec_pt;             // [n_obs] point row
    int32_t* rec_flags;          // [n_obs]
    int32_t* rec_free;           // [n_obs] column block in S, -1: none this phase
    int32_t* kf_free;            // [n_kf] column block in S, -1: none this phase
    int32_t* kf_elist;           // [n_obs] the edges of each free keyframe, in edge order
    int32_t* pt_active;          // [n_pt]
};
size_t local_ba_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs, int max_free);
hipError_t launch_local_ba(LocalBaArgs A, int batch, char* workspace, hipStream_t stream);

// k_global_ba (orbx_globalba.hip): Optimizer::BundleAdjustment for `batch` maps, one workgroup
// each; everything sized by a problem's keyframes, points or observations, and the block
// envelope of the reduced system S, lives in the workspace.
struct GlobalBaArgs {
    const int32_t* kf_off;       // [B + 1]
    int n_kf;
    const float* kf_Tcw;         // [n_kf][12]
    const uint8_t* kf_fixed;     // [n_kf]
    const int32_t* kf_slot;      // [n_kf]
    const int32_t* pt_off;       // [B + 1]
    int n_pt;
    const float* pt_pos;         // [n_pt][3]
    const int32_t* obs_off;      // [n_pt + 1]
    int n_obs;
    const int32_t* obs_kf;       // [n_obs]
    const int32_t* obs_kp;       // [n_obs]
    int n_slots, cap;
    const orbx_keypoint* kps;    // [n_slots][cap]
    const float* u_right;        // [n_slots][cap] or null
    float inv_sigma2[ORBX_MAX_LEVELS];
    int nlevels;
    float fx, fy, cx, cy, bf;
    float delta_mono, delta_stereo;
    int iterations, robust, dense;
    long long max_env_blocks;    // 6 x 6 blocks per problem that S is sized for
    float* kf_Tcw_out;           // [n_kf][12]
    float* pt_pos_out;           // [n_pt][3]
    uint8_t* pt_included;        // [n_pt]
    int32_t* trace;              // [B][2] or null
    double* chi2;                // [B][2] or null
    int32_t* status;             // [B]
    // set by launch_global_ba
    double* pose;                // [n_kf][2][16]: current and trial {q xyzw, t, R row by row}
    double* pt;                  // [n_pt][2][3]: current and trial
    double* pt_sys;              // [n_pt][24]: Hll (6), bl (3), Dinv (9), Dinv bl (3), xl (3)
    double* W;                   // [n_obs][18]: A^T (rho' Omega) B
    double* L;                   // [B][max_env_blocks][36]: S, factored in place
    double* hpp;                 // [n_kf][21]: the upper triangle of a block column's Hpp
    double* vec;                 // [n_kf][5][6]: b_p, b_s, x and the two work vectors of the solve
    long long* col_off;          // [n_kf + B] first block of a column (F + 1 per problem)
    long long* row_off;          // [n_kf + B] first entry of a block row in rows
    float* rec;                  // [n_obs][4]: u, v, u_right, invSigma2
    int32_t* rows;               // [B][max_env_blocks] the columns of every block row
    int32_t* rec_kf;             // [n_obs] keyframe row, -1: not an edge
    int32_t* rec_pt;             // [n_obs] point row
    int32_t* rec_flags;          // [n_obs]
    int32_t* rec_free;           // [n_obs] block column in S, -1: none
    int32_t* kf_elist;           // [n_obs] the edges of each block column, in edge order
    int32_t* kf_free;            // [n_kf] block column in S, -1: none
    int32_t* free_kf;            // [n_kf] its inverse
    int32_t* deg;                // [n_kf] counters
    int32_t* first;              // [n_kf + B]
    int32_t* eoff;               // [n_kf + B] first edge of a block column in kf_elist
    int32_t* pt_active;          // [n_pt]
};
size_t global_ba_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs, long long max_env_blocks);
hipError_t launch_global_ba(GlobalBaArgs A, int batch, char* workspace, hipStream_t stream);

// k_essential_graph (orbx_essgraph.hip): Optimizer::OptimizeEssentialGraph for `batch` maps,
// one workgroup each; the estimates, the measurements, the Jacobians, the block envelope of H,
// its factor and every vector live in the workspace.
struct EssGraphArgs {
    const int32_t* kf_off;       // [B + 1]
    int n_kf;
    const float* kf_Tcw;         // [n_kf][12]
    const int32_t* kf_corr;      // [n_kf] row of corr_S or -1
    const double* corr_S;        // [n_corr][8]
    int n_corr;
    const int32_t* loop_kf;      // [B]
    const int32_t* edge_off;     // [B + 1]
    int n_edges;
    const int32_t* edge_v;       // [n_edges][2]
    const int32_t* edge_kind;    // [n_edges]
    const int32_t* pt_off;       // [B + 1]
    int n_pt;
    const float* pt_pos;         // [n_pt][3]
    const int32_t* pt_ref;       // [n_pt]
    int fix_scale, iterations, dense;
    long long max_env_blocks;    // blocks per problem that H and its factor are sized for
    float* kf_Tcw_out;           // [n_kf][12]
    float* pt_pos_out;           // [n_pt][3]
    double* Scw_out;             // [n_kf][8] or null
    int32_t* trace;              // [B][2] or null
    double* chi2;                // [B][2] or null
    int32_t* status;             // [B]
    // set by launch_essential_graph
    long long* ticks;            // [B][2] wall-clock ticks {linearisations, solves}; null unless "essgraph_stamps"
    double probes[14 * 8];       // Sim3(+-1e-9 e_d) as q xyzw, t, s
    double* S;                   // [n_kf][3][8]: vScw, the estimate, its backup
    double* meas;                // [n_edges][8]
    double* J;                   // [n_edges][2][49]
    double* err;                 // [n_edges][7]
    double* H;                   // [B][max_env_blocks][49]
    double* L;                   // [B][max_env_blocks][49]
    double* vec;                 // [n_kf][4][7]: b, x, and the two work vectors of the solve
    long long* col_off;          // [n_kf + B] first block of a column (F + 1 per problem)
    long long* row_off;          // [n_kf + B] first entry of a block row in rows
    int32_t* rows;               // [B][max_env_blocks] the columns of every block row
    int32_t* edge_ok;            // [n_edges]
    int32_t* free_idx;           // [n_kf] index among the vertices that may move, -1: none
    int32_t* free_kf;            // [n_kf] its inverse
    int32_t* first;              // [n_kf + B]
    int32_t* adj_off;            // [n_kf + B]
    int32_t* adj;                // [n_edges][2]: 2 e + side, per vertex in edge order
    int32_t* deg;                // [n_kf]
};
size_t essential_graph_workspace_bytes(int batch, int n_kf, int n_edges, long long max_env_blocks);
hipError_t launch_essential_graph(EssGraphArgs A, int batch, char* workspace, hipStream_t stream);

// k_triangulate_pairs (orbx_triangulate.hip): LocalMapping::CreateNewMapPoints' triangulation
// and tests (LocalMapping.cc:307-501) over the matched pairs of `npairs` keyframe pairs, one
// workgroup each.
struct TriGeomKF {
    const orbx_keypoint* keys_un;  // mvKeysUn
    const orbx_keypoint* keys;     // mvKeys or null (= keys_un)
    const float* u_right;          // mvuRight or null (monocular)
    const float* depth;            // mvDepth or null (mbf / (mvKeys.x - mvuRight) in float)
    const int32_t* n;              // N (one device int)
    float Tcw[12];
    double Ow[3];                  // -Rcw^T tcw in double (the host builds it)
};
struct TriGeomArgs {
    const TriGeomKF* kfs;
    const int32_t* pair_kf;        // [P][2] keyframe records of KF1, KF2
    const int32_t* pairs;          // [P][cap][2] vMatchedPairs
    const int32_t* npairs;         // [P]
    int cap;                       // pair slots per row
    int kcap;                      // keypoint slots per keyframe (N is clamped into [0, kcap])
    float fx, fy, cx, cy, mb, mbf;
    int nlevels;
    float scale_factor;            // mfScaleFactor
    const float* scale;            // [nlevels] mvScaleFactors (device)
    const float* sigma2;           // [nlevels] mvLevelSigma2 (device)
    uint8_t* reason;               // every output: [P][cap]... or null
    uint8_t* method;
    float* pos;
    float* normal;
    float* max_distance;
    float* min_distance;
    int32_t* nnew;                 // [P]
    int32_t* new_idx;              // [P][cap]
};
hipError_t launch_triangulate_pairs(const TriGeomArgs& A, int npairs, hipStream_t stream);

hipError_t launch_window_match(const uint8_t* qdesc, int nq, const uint8_t* tdesc, const int32_t* tlevel,
                               const int32_t* cand_off, const int32_t* cand, int tie_last,
                               int32_t* best_idx, int32_t* best_dist, int32_t* best_level,
                               int32_t* second_dist, int32_t* second_level, hipStream_t stream);

}  // namespace orbx
