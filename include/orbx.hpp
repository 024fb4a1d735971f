// orbx.hpp -- header-only C++ mirror of ORB_SLAM2::ORBextractor / ORBmatcher /
// ORBVocabulary / KeyFrameDatabase over the C ABI in orbx.h (liborbx.so).  Same class
// names, constructor arguments, call operator, getters and search entry points as
// include/ORBextractor.h:76-220, include/ORBmatcher.h:47-228 and
// include/KeyFrameDatabase.h:40-92 of the reference, with OpenCV types replaced by plain
// containers (cv::KeyPoint == orbx_keypoint, 28 bytes; descriptor rows of 32 bytes).
// Errors throw orbx::Error on this side of the boundary; nothing throws across it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbx.h"

namespace orbx {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc) {
    if (rc != ORBX_OK && rc != ORBX_EMPTY) throw Error(rc, std::string("orbx: ") + orbx_last_error());
}

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
        : nlevels_(nlevels), scaleFactor_(scaleFactor) {
        orbx_extractor_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
        check(orbx_extractor_create(&p, device, &h_));
    }
    ~ORBextractor() { orbx_extractor_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // operator()(image, mask, keypoints, descriptors): an empty image leaves the outputs
    // untouched (ORBextractor.cc:1517-1518); zero keypoints empty the descriptors.
    void operator()(const uint8_t* img, int width, int height, size_t stride, std::vector<orbx_keypoint>& keypoints,
                    std::vector<uint8_t>& descriptors) {
        if (!img || width <= 0 || height <= 0) return;
        int cap = 0;
        check(orbx_extractor_max_keypoints(h_, width, height, &cap));
        keypoints.resize((size_t)cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(orbx_extract(h_, img, width, height, stride, keypoints.data(), descriptors.data(), cap, &n));
        keypoints.resize((size_t)n);
        descriptors.resize((size_t)n * 32);
    }

    int GetLevels() const { return nlevels_; }
    float GetScaleFactor() const { return scaleFactor_; }
    std::vector<float> GetScaleFactors() const { return levels(0); }
    std::vector<float> GetInverseScaleFactors() const { return levels(1); }
    std::vector<float> GetScaleSigmaSquares() const { return levels(2); }
    std::vector<float> GetInverseScaleSigmaSquares() const { return levels(3); }

    // mvImagePyramid[level] of the last call (ROI only), row-major w x h
    std::vector<uint8_t> ImagePyramidLevel(int level, int* w, int* h, int frame = 0) {
        check(orbx_pyramid_level(h_, frame, level, nullptr, 0, w, h));
        std::vector<uint8_t> out((size_t)(*w) * (*h));
        check(orbx_pyramid_level(h_, frame, level, out.data(), (size_t)*w, nullptr, nullptr));
        return out;
    }

    orbx_extractor* handle() { return h_; }

private:
    std::vector<float> levels(int which) const {
        std::vector<float> a(nlevels_), b(nlevels_), c(nlevels_), d(nlevels_);
        check(orbx_extractor_levels(h_, nullptr, a.data(), b.data(), c.data(), d.data()));
        return which == 0 ? a : which == 1 ? b : which == 2 ? c : d;
    }
    orbx_extractor* h_ = nullptr;
    int nlevels_;
    float scaleFactor_;
};

class ORBmatcher {
public:
    static const int TH_HIGH = 100;
    static const int TH_LOW = 50;
    static const int HISTO_LENGTH = 30;

    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0) {
        check(orbx_matcher_create(device, nnratio, checkOri ? 1 : 0, &h_));
    }
    ~ORBmatcher() { orbx_matcher_destroy(h_); }
    ORBmatcher(const ORBmatcher&) = delete;
    ORBmatcher& operator=(const ORBmatcher&) = delete;

    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orbx_hamming(a, b); }

    // The four SearchByProjection overloads: the searched frame (F, CurrentFrame, KF) holds at
    // most 8191 keypoints -- 8192 or more throws before anything is uploaded
    // (ORBX_ERR_UNSUPPORTED), the caller's arrays untouched; the number of queries
    // (vpMapPoints, the last frame's / keyframe's keypoints, vpPoints) is bounded only by memory.

    // SearchByProjection(Frame&, const vector<MapPoint*>&, th)
    int SearchByProjection(const orbx_frame_view& F, int32_t* mvpMapPoints, const std::vector<int32_t>& vpMapPoints,
                           const orbx_mappoints& mps, const orbx_track& trk, float th = 3) {
        int n = 0;
        check(orbx_search_by_projection_local(h_, &F, mvpMapPoints, vpMapPoints.data(), (int)vpMapPoints.size(), &mps,
                                              &trk, th, &n));
        return n;
    }

    // SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
    int SearchByProjection(const orbx_frame_view& CurrentFrame, int32_t* curMapPoints, const orbx_frame_view& LastFrame,
                           const int32_t* lastMapPoints, const uint8_t* lastOutlier, const orbx_mappoints& mps,
                           float th, bool bMono) {
        int n = 0;
        check(orbx_search_by_projection_frame(h_, &CurrentFrame, curMapPoints, &LastFrame, lastMapPoints, lastOutlier,
                                              &mps, th, bMono ? 1 : 0, &n));
        return n;
    }

    // SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
    int SearchByProjection(const orbx_frame_view& CurrentFrame, int32_t* curMapPoints, const orbx_frame_view& KF,
                           const int32_t* kfMapPoints, const uint8_t* alreadyFound, const orbx_mappoints& mps,
                           float th, int ORBdist) {
        int n = 0;
        check(orbx_search_by_projection_keyframe(h_, &CurrentFrame, curMapPoints, &KF, kfMapPoints, alreadyFound, &mps,
                                                 th, ORBdist, &n));
        return n;
    }

    // SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>& vpMatched, th)
    int SearchByProjection(const orbx_frame_view& KF, const float Scw[12], const std::vector<int32_t>& vpPoints,
                           int32_t* vpMatched, const orbx_mappoints& mps, int th) {
        int n = 0;
        check(orbx_search_by_projection_sim3(h_, &KF, Scw, vpPoints.data(), (int)vpPoints.size(), vpMatched, &mps, th,
                                             &n));
        return n;
    }

    // SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
    struct FeatureVector {
        std::vector<int32_t> node, off, idx;  // CSR of DBoW2::FeatureVector
    };
    int SearchForTriangulation(const orbx_frame_view& KF1, const uint8_t* kf1HasMP, const FeatureVector& fv1,
                               const orbx_frame_view& KF2, const uint8_t* kf2HasMP, const FeatureVector& fv2,
                               const float F12[9], std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                               bool bOnlyStereo) {
        std::vector<int32_t> pairs((size_t)KF1.n * 2 + 2);
        int np = 0;
        check(orbx_search_for_triangulation(h_, &KF1, kf1HasMP, fv1.node.data(), fv1.off.data(), fv1.idx.data(),
                                            (int)fv1.node.size(), &KF2, kf2HasMP, fv2.node.data(), fv2.off.data(),
                                            fv2.idx.data(), (int)fv2.node.size(), F12, bOnlyStereo ? 1 : 0,
                                            pairs.data(), &np));
        vMatchedPairs.clear();
        for (int i = 0; i < np; i++) vMatchedPairs.emplace_back((size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]);
        return np;
    }

    // SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches); kfMapPoints: id or -1
    int SearchByBoW(const orbx_frame_view& KF, const int32_t* kfMapPoints, const FeatureVector& kfFeatVec,
                    const orbx_frame_view& F, const FeatureVector& fFeatVec, std::vector<int32_t>& vpMapPointMatches) {
        vpMapPointMatches.assign((size_t)F.n, -1);
        int n = 0;
        check(orbx_search_by_bow_frame(h_, &KF, kfMapPoints, kfFeatVec.node.data(), kfFeatVec.off.data(),
                                       kfFeatVec.idx.data(), (int)kfFeatVec.node.size(), &F, fFeatVec.node.data(),
                                       fFeatVec.off.data(), fFeatVec.idx.data(), (int)fFeatVec.node.size(),
                                       vpMapPointMatches.data(), &n));
        return n;
    }

    // SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
    int SearchByBoW(const orbx_frame_view& KF1, const int32_t* mapPoints1, const FeatureVector& fv1,
                    const orbx_frame_view& KF2, const int32_t* mapPoints2, const FeatureVector& fv2,
                    std::vector<int32_t>& vpMatches12) {
        vpMatches12.assign((size_t)KF1.n, -1);
        int n = 0;
        check(orbx_search_by_bow_keyframes(h_, &KF1, mapPoints1, fv1.node.data(), fv1.off.data(), fv1.idx.data(),
                                           (int)fv1.node.size(), &KF2, mapPoints2, fv2.node.data(), fv2.off.data(),
                                           fv2.idx.data(), (int)fv2.node.size(), vpMatches12.data(), &n));
        return n;
    }

    // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize); vbPrevMatched as x,y pairs
    int SearchForInitialization(const orbx_frame_view& F1, const orbx_frame_view& F2, std::vector<float>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10) {
        vnMatches12.assign((size_t)F1.n, -1);
        int n = 0;
        check(orbx_search_for_initialization(h_, &F1, &F2, vbPrevMatched.data(), vnMatches12.data(), windowSize, &n));
        return n;
    }

    // Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th): search part, best[k] = KF keypoint or -1
    void Fuse(const orbx_frame_view& KF, const std::vector<int32_t>& vpMapPoints, const uint8_t* skip,
              const orbx_mappoints& mps, std::vector<int32_t>& best, float th = 3.0f) {
        best.assign(vpMapPoints.size(), -1);
        check(orbx_fuse(h_, &KF, vpMapPoints.data(), (int)vpMapPoints.size(), skip, &mps, th, best.data()));
    }

    // Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint): search part
    void Fuse(const orbx_frame_view& KF, const float Scw[12], const std::vector<int32_t>& vpPoints, const uint8_t* skip,
              const orbx_mappoints& mps, std::vector<int32_t>& best, float th = 4.0f) {
        best.assign(vpPoints.size(), -1);
        check(orbx_fuse_sim3(h_, &KF, Scw, vpPoints.data(), (int)vpPoints.size(), skip, &mps, th, best.data()));
    }

    // SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
    int SearchBySim3(const orbx_frame_view& KF1, const int32_t* mapPoints1, const uint8_t* alreadyMatched1,
                     const orbx_frame_view& KF2, const int32_t* mapPoints2, const uint8_t* alreadyMatched2,
                     const orbx_mappoints& mps, float s12, const float R12[9], const float t12[3], float th,
                     int32_t* vpMatches12) {
        int n = 0;
        check(orbx_search_by_sim3(h_, &KF1, mapPoints1, alreadyMatched1, &KF2, mapPoints2, alreadyMatched2, &mps, s12,
                                  R12, t12, th, vpMatches12, &n));
        return n;
    }

    orbx_matcher* handle() { return h_; }

private:
    orbx_matcher* h_ = nullptr;
};

// The RGB-D Frame constructor's steps after ExtractORB (Frame.cc:192-264, 227-230):
// UndistortKeyPoints (Frame.cc:586-628) and ComputeStereoFromRGBD (Frame.cc:888-909) over
// the depth image as GrabImageRGBD receives it -- ORBX_DEPTH_U16 (the library applies
// mDepthMapFactor, Tracking.cc:265-271) or ORBX_DEPTH_F32 -- with mDepthMapFactor =
// 1 / DepthMapFactor (Tracking.cc:166-170) and mbf.  mvuRight / mvDepth are -1 where the
// depth is not positive, as the reference's vectors are initialised.
inline void ComputeStereoFromRGBD(const orbx_camera& cam, const std::vector<orbx_keypoint>& mvKeys,
                                  const void* depth, int depthType, int width, int height, size_t rowBytes,
                                  float mDepthMapFactor, float mbf, std::vector<orbx_keypoint>& mvKeysUn,
                                  std::vector<float>& mvuRight, std::vector<float>& mvDepth, int device = 0) {
    const int n = (int)mvKeys.size();
    mvKeysUn.resize((size_t)n);
    mvuRight.assign((size_t)n, -1.0f);
    mvDepth.assign((size_t)n, -1.0f);
    check(orbx_compute_stereo_from_rgbd(device, &cam, mvKeys.data(), n, depth, depthType, width, height, rowBytes,
                                        mDepthMapFactor, mbf, mvKeysUn.data(), mvuRight.data(), mvDepth.data()));
}

// The covisibility graph (KeyFrame::UpdateConnections and the lists it keeps, src/KeyFrame.cc:
// 139-229, 324-415, 506-520) over keyframe ids in [0, maxKeyFrames): a KeyFrame* is its mnId,
// a MapPoint* its id.  The map is mvpMapPoints as a [keyframes][cap] id table (-1 = NULL).
class Covisibility {
public:
    Covisibility(int maxKeyFrames, int cap, int maxMapPoints, int maxConnections = 256, int device = 0)
        : maxConn_(maxConnections) {
        check(orbx_covis_create(device, maxKeyFrames, cap, maxMapPoints, maxConnections, &h_));
    }
    ~Covisibility() { orbx_covis_destroy(h_); }
    Covisibility(const Covisibility&) = delete;
    Covisibility& operator=(const Covisibility&) = delete;

    // MapPoint::GetObservations() of every point from the keyframes' mvpMapPoints: device
    // tables (they must outlive the later calls) ...
    void RefreshObservations(int nKeyFrames, const int32_t* d_kf_mp, const int32_t* d_kf_n, const uint8_t* d_kf_bad,
                             int nMapPoints, const uint8_t* d_mp_bad, void* stream = nullptr) {
        check(orbx_covis_refresh_observations_device(h_, nKeyFrames, d_kf_mp, d_kf_n, d_kf_bad, nMapPoints, d_mp_bad,
                                                     stream));
    }
    // ... or host vectors (kfBad / mpBad may be empty: nothing is bad)
    void RefreshObservations(const std::vector<int32_t>& kfMapPoints, const std::vector<int32_t>& kfN,
                             const std::vector<uint8_t>& kfBad, int nMapPoints, const std::vector<uint8_t>& mpBad) {
        check(orbx_covis_refresh_observations(h_, (int)kfN.size(), kfMapPoints.data(), kfN.data(),
                                              kfBad.empty() ? nullptr : kfBad.data(), nMapPoints,
                                              mpBad.empty() ? nullptr : mpBad.data()));
    }
    // pKF->UpdateConnections() for each of ids, in order
    void UpdateConnections(const std::vector<int32_t>& ids, void* stream = nullptr) {
        check(orbx_covis_update_connections_device(h_, ids.data(), (int)ids.size(), stream));
    }
    void UpdateConnections(int id) { UpdateConnections(std::vector<int32_t>{id}); }
    // the connection part of pKF->SetBadFlag()
    void EraseKeyFrame(int id, void* stream = nullptr) { check(orbx_covis_erase_keyframe_device(h_, id, stream)); }
    // pKF->SetBadFlag() for each of ids, in order, on the device tables of the last refresh (also
    // SetErase() once the caller cleared mbNotErase): connections, observations, the MapPoints
    // that fall to nObs <= 2, the children's new parents, mbBad.  The results are device ints.
    void SetBadFlag(const orbx_map_tables& maps, const std::vector<int32_t>& ids, int32_t* d_nNewBadMapPoints,
                    int32_t* d_status, void* stream = nullptr) {
        check(orbx_covis_set_bad_flag_device(h_, &maps, ids.data(), (int)ids.size(), d_nNewBadMapPoints, d_status, stream));
    }
    // LocalMapping::KeyFrameCulling() for mpCurrentKeyFrame = curKF; every result is a device array
    struct CullResult {
        int32_t *cand, *candCounts, *nCand, *culled, *nCulled, *nNewBadMapPoints, *status;
    };
    void KeyFrameCulling(const orbx_map_tables& maps, int curKF, bool mbMonocular, const CullResult& r,
                         void* stream = nullptr) {
        check(orbx_keyframe_culling_device(h_, &maps, curKF, mbMonocular ? 1 : 0, r.cand, r.candCounts, r.nCand, r.culled,
                                           r.nCulled, r.nNewBadMapPoints, r.status, stream));
    }
    // LocalMapping::MapPointCulling() over mlpRecentAddedMapPoints (d_recent / d_nRecent, in/out)
    void MapPointCulling(const orbx_map_tables& maps, int nCurrentKFid, bool mbMonocular, int32_t* d_recent,
                         int32_t* d_nRecent, int maxRecent, const int32_t* d_mnFirstKFid, const int32_t* d_mnFound,
                         const int32_t* d_mnVisible, int32_t* d_nCulled, void* stream = nullptr) {
        check(orbx_map_point_culling_device(h_, &maps, nCurrentKFid, mbMonocular ? 1 : 0, d_recent, d_nRecent, maxRecent,
                                            d_mnFirstKFid, d_mnFound, d_mnVisible, d_nCulled, stream));
    }
    // MapPoint::Observations() of every MapPoint
    void ObservationCounts(const float* d_mvuRight, int32_t* d_out, void* stream = nullptr) {
        check(orbx_covis_observation_counts_device(h_, d_mvuRight, d_out, stream));
    }
    // vector<KeyFrame*> GetVectorCovisibleKeyFrames(); weights: mvOrderedWeights
    std::vector<int32_t> GetVectorCovisibleKeyFrames(int id, std::vector<int32_t>* weights = nullptr) {
        std::vector<int32_t> kf((size_t)maxConn_), w((size_t)maxConn_);
        int n = 0;
        check(orbx_covis_ordered(h_, id, kf.data(), w.data(), maxConn_, &n));
        kf.resize((size_t)n);
        w.resize((size_t)n);
        if (weights) *weights = w;
        return kf;
    }
    std::vector<int32_t> GetBestCovisibilityKeyFrames(int id, int N) {
        std::vector<int32_t> kf = GetVectorCovisibleKeyFrames(id);
        if ((int)kf.size() >= N) kf.resize((size_t)(N < 0 ? 0 : N));
        return kf;
    }
    std::vector<int32_t> GetCovisiblesByWeight(int id, int w) {
        std::vector<int32_t> ws, kf = GetVectorCovisibleKeyFrames(id, &ws);
        if (kf.empty()) return kf;
        const auto it = std::upper_bound(ws.begin(), ws.end(), w, [](int a, int b) { return a > b; });
        if (it == ws.end() && ws.back() < w) return {};
        kf.resize((size_t)(it - ws.begin()));
        return kf;
    }
    orbx_covis_view View() {
        orbx_covis_view v{};
        check(orbx_covis_view_device(h_, &v));
        return v;
    }
    orbx_covis* handle() { return h_; }

private:
    orbx_covis* h_ = nullptr;
    int maxConn_;
};

// LoopClosing::CorrectLoop on a Covisibility graph whose map tables live on the device
// (src/LoopClosing.cc:482-571, 595-618; the tables of Optimizer::OptimizeEssentialGraph,
// src/Optimizer.cc:913-1089, 1125-1133; MapPoint::UpdateNormalAndDepth, src/MapPoint.cc:386-439).
// Every array of the structs is a device array except scale_factors; nothing is read back.
class LoopClosing {
public:
    explicit LoopClosing(Covisibility& graph) : g_(graph) {}

    // CorrectLoop() up to the fusion: UpdateConnections, the Sim3 propagation, the first
    // correction of the MapPoints with their UpdateNormalAndDepth, SetPose, UpdateConnections
    void CorrectLoopPropagate(const orbx_correct_loop_propagate& a, void* stream = nullptr) {
        check(orbx_correct_loop_propagate_device(g_.handle(), &a, stream));
    }
    // after the caller's SearchAndFuse and RefreshObservations: LoopConnections and the tables of
    // one orbx_essential_graph_batch problem
    void AssembleEssentialGraph(const orbx_essential_graph_assembly& a, void* stream = nullptr) {
        check(orbx_essential_graph_assemble_device(g_.handle(), &a, stream));
    }
    // pMP->UpdateNormalAndDepth() for d_ids[0 .. nIds), or for every MapPoint when d_ids is null
    void UpdateNormalAndDepth(const orbx_normal_depth& a, const int32_t* d_ids, int nIds, int32_t* d_status,
                              void* stream = nullptr) {
        check(orbx_update_normal_and_depth_device(g_.handle(), &a, d_ids, nIds, d_status, stream));
    }

private:
    Covisibility& g_;
};

// Tracking's local map (src/Tracking.cc:1342-1500) and TrackLocalMap's tally (cc:1047-1081) on a
// Covisibility graph: frames are rows of a [frames][cap] MapPoint id table (-1 = NULL).
class Tracking {
public:
    explicit Tracking(Covisibility& graph) : g_(graph) {}

    // mvpLocalKeyFrames / mpReferenceKF / mvpLocalMapPoints of a batch of frames; the first three
    // are in/out and persist from call to call (an empty counter keeps them)
    struct LocalMaps {
        int maxLocalKeyFrames = 0;
        std::vector<int32_t> localKeyFrames;   // [frames][maxLocalKeyFrames]
        std::vector<int32_t> nLocalKeyFrames;  // [frames]
        std::vector<int32_t> referenceKF;      // [frames]
        std::vector<int32_t> localOff;         // [frames + 1]
        std::vector<int32_t> localMapPoints;   // frame b: [localOff[b], localOff[b + 1])
        std::vector<int32_t> counts, status;   // [frames][2], [frames] ORBX_LOCAL_MAP_STATUS_*
    };

    // UpdateLocalMap() on device arrays: everything is written there, nothing is read back
    void UpdateLocalMap(const orbx_local_map_update& u, void* stream = nullptr) {
        check(orbx_update_local_map_device(g_.handle(), &u, stream));
    }
    // ... or on host vectors: mvpMapPoints [frames][cap] (bad MapPoints become -1), N [frames];
    // parent empty: the graph's own mpParent.  lm is (re)initialised when its shape differs.
    void UpdateLocalMap(std::vector<int32_t>& mvpMapPoints, const std::vector<int32_t>& N, int cap, LocalMaps& lm,
                        int maxLocalKeyFrames, int maxLocalPoints, int maxTotal,
                        const std::vector<int32_t>& parent = std::vector<int32_t>()) {
        const size_t B = N.size();
        if (lm.maxLocalKeyFrames != maxLocalKeyFrames || lm.nLocalKeyFrames.size() != B) {
            lm.maxLocalKeyFrames = maxLocalKeyFrames;
            lm.localKeyFrames.assign(B * (size_t)maxLocalKeyFrames, -1);
            lm.nLocalKeyFrames.assign(B, 0);
            lm.referenceKF.assign(B, -1);
        }
        lm.localOff.assign(B + 1, 0);
        lm.localMapPoints.assign((size_t)maxTotal, -1);
        lm.counts.assign(2 * B, 0);
        lm.status.assign(B, 0);
        orbx_local_map_update u{};
        u.batch = (int)B;
        u.cap = cap;
        u.frame_mp = mvpMapPoints.data();
        u.n = N.data();
        u.parent = parent.empty() ? nullptr : parent.data();
        u.max_local_kf = maxLocalKeyFrames;
        u.max_local_points = maxLocalPoints;
        u.max_total = maxTotal;
        u.local_kf = lm.localKeyFrames.data();
        u.local_kf_n = lm.nLocalKeyFrames.data();
        u.ref_kf = lm.referenceKF.data();
        u.local_off = lm.localOff.data();
        u.local_ids = lm.localMapPoints.data();
        u.counts = lm.counts.data();
        u.status = lm.status.data();
        check(orbx_update_local_map(g_.handle(), &u));
        lm.localMapPoints.resize((size_t)lm.localOff[B]);
    }

    // SearchLocalPoints() on the lists that UpdateLocalMap wrote on the device
    static void SearchLocalPoints(ORBmatcher& matcher, const orbx_mappoints_device& mps, const orbx_local_map_batch& lm,
                                  const int32_t* d_local_off, int maxLocalPoints, int maxTotal, void* stream = nullptr) {
        check(orbx_search_local_points_offsets_device(matcher.handle(), &mps, &lm, d_local_off, maxLocalPoints, maxTotal,
                                                      stream));
    }

    // mnMatchesInliers and TrackLocalMap's verdict after the second PoseOptimization
    void TrackLocalMapTally(const orbx_track_local_map_tally& t, void* stream = nullptr) {
        check(orbx_track_local_map_tally_device(g_.handle(), &t, stream));
    }

private:
    Covisibility& g_;
};

// Optimizer (include/Optimizer.h): the g2o call on the per-frame path, the one of
// LoopClosing::ComputeSim3 and the one of LocalMapping::Run.
// PoseOptimization(Frame*) (src/Optimizer.cc:299-502) on the Frame's arrays: mvKeysUn,
// mvuRight (empty: monocular), mvpMapPoints as MapPoint ids (-1 = NULL) into the positions
// mpPos (GetWorldPos(), 3 floats per id), mvInvLevelSigma2, fx fy cx cy mbf and mTcw (rows
// 0..2, 12 floats, updated in place as SetPose does).  mvbOutlier is resized to the keypoints
// and updated; returns nInitialCorrespondences - nBad.  trace (optional, 8 ints): per round
// the LM iterations run and the linear solves tried.  Runs on the matcher's handle and stream.
class Optimizer {
public:
    static int PoseOptimization(ORBmatcher& matcher, const std::vector<orbx_keypoint>& mvKeysUn,
                                const std::vector<float>& mvuRight, const std::vector<int32_t>& mvpMapPoints,
                                const std::vector<float>& mpPos, const std::vector<float>& mvInvLevelSigma2, float fx,
                                float fy, float cx, float cy, float mbf, float* mTcw, std::vector<uint8_t>& mvbOutlier,
                                int32_t* trace = nullptr, int* nInitialCorrespondences = nullptr) {
        const int n = (int)mvKeysUn.size();
        mvbOutlier.resize((size_t)n, 0);
        float out[12];
        int inliers = 0;
        check(orbx_pose_optimization(matcher.handle(), mvKeysUn.data(), n, mvuRight.empty() ? nullptr : mvuRight.data(),
                                     mvpMapPoints.data(), mpPos.data(), (int)(mpPos.size() / 3),
                                     mvInvLevelSigma2.data(), (int)mvInvLevelSigma2.size(), fx, fy, cx, cy, mbf, mTcw,
                                     out, mvbOutlier.data(), nInitialCorrespondences, trace, &inliers));
        for (int i = 0; i < 12; i++) mTcw[i] = out[i];
        return inliers;
    }

    // OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:1173-1358)
    // on the keyframes' arrays: mvKeysUn1 / mvKeysUn2, pKF1's GetMapPointMatches() and
    // vpMatches1 as MapPoint ids (-1 = NULL or isBad()) into mpPos, idx2[i] =
    // vpMatches1[i]->GetIndexInKeyFrame(pKF2), the poses' rows 0..2, mvInvLevelSigma2 and fx fy
    // cx cy of either keyframe.  g2oS12 is R12 (9) / t12 (3) / s12, updated in place unless 0 is
    // returned; rejected vpMatches1 entries become -1.  Returns nIn.  trace (optional, 4 ints):
    // per optimisation the LM iterations run and the linear solves tried.
    static int OptimizeSim3(ORBmatcher& matcher, const std::vector<orbx_keypoint>& mvKeysUn1,
                            const std::vector<int32_t>& vpMapPoints1, std::vector<int32_t>& vpMatches1,
                            const std::vector<int32_t>& idx2, const std::vector<orbx_keypoint>& mvKeysUn2,
                            const std::vector<float>& mpPos, const float* Tcw1, const float* Tcw2,
                            const std::vector<float>& mvInvLevelSigma2_1, const std::vector<float>& mvInvLevelSigma2_2,
                            const float* K1, const float* K2, float* R12, float* t12, float* s12, float th2,
                            bool bFixScale, int32_t* trace = nullptr, int* nCorrespondences = nullptr,
                            int* nBad = nullptr) {
        const int32_t n1 = (int32_t)vpMatches1.size(), n2 = (int32_t)mvKeysUn2.size();
        if (mvKeysUn1.size() != (size_t)n1 || vpMapPoints1.size() != (size_t)n1 || idx2.size() != (size_t)n1 ||
            mvInvLevelSigma2_1.size() != mvInvLevelSigma2_2.size())
            throw std::runtime_error("OptimizeSim3: array sizes differ");
        // the call takes no null array: an empty one gets one spare element
        const orbx_keypoint kp0{};
        const int32_t i0 = -1;
        int32_t m0 = -1;
        const float p0[3] = {0.0f, 0.0f, 0.0f};
        float Ro[9], to[3], so = 0.0f;
        int32_t counts[3] = {0, 0, 0};
        orbx_optimize_sim3_batch q{};
        q.batch = 1;
        q.cap1 = n1 > 0 ? n1 : 1;
        q.n1 = &n1;
        q.kps1 = n1 > 0 ? mvKeysUn1.data() : &kp0;
        q.mp1 = n1 > 0 ? vpMapPoints1.data() : &i0;
        q.matches12 = n1 > 0 ? vpMatches1.data() : &m0;
        q.idx2 = n1 > 0 ? idx2.data() : &i0;
        q.cap2 = n2 > 0 ? n2 : 1;
        q.n2 = &n2;
        q.kps2 = n2 > 0 ? mvKeysUn2.data() : &kp0;
        q.n_mp = (int)(mpPos.size() / 3);
        q.mp_pos = q.n_mp > 0 ? mpPos.data() : p0;
        q.Tcw1 = Tcw1;
        q.Tcw2 = Tcw2;
        q.inv_level_sigma2_1 = mvInvLevelSigma2_1.data();
        q.inv_level_sigma2_2 = mvInvLevelSigma2_2.data();
        q.nlevels = (int)mvInvLevelSigma2_1.size();
        q.K1 = K1;
        q.K2 = K2;
        q.R12 = R12;
        q.t12 = t12;
        q.s12 = s12;
        q.th2 = th2;
        q.fix_scale = bFixScale ? 1 : 0;
        q.R12_opt = Ro;
        q.t12_opt = to;
        q.s12_opt = &so;
        q.ninliers = &counts[0];
        q.ncorr = &counts[1];
        q.nbad = &counts[2];
        q.trace = trace;
        check(orbx_optimize_sim3(matcher.handle(), &q));
        for (int i = 0; i < 9; i++) R12[i] = Ro[i];
        for (int i = 0; i < 3; i++) t12[i] = to[i];
        *s12 = so;
        if (nCorrespondences) *nCorrespondences = counts[1];
        if (nBad) *nBad = counts[2];
        return counts[0];
    }

    // LocalBundleAdjustment's covisibility walk and edge walk (src/Optimizer.cc:526-583, 656-760)
    // for the current keyframes a.cur_kf on the graph, into the device tables of
    // orbx_local_ba_batch (see orbx_local_ba_assemble_device), and the way back (cc:828-853).
    static void AssembleLocalBundleAdjustment(Covisibility& graph, const orbx_local_ba_assembly& a, void* stream = nullptr) {
        check(orbx_local_ba_assemble_device(graph.handle(), &a, stream));
    }
    static void ApplyLocalBundleAdjustment(Covisibility& graph, const orbx_local_ba_apply& a, void* stream = nullptr) {
        check(orbx_local_ba_apply_device(graph.handle(), &a, stream));
    }

    // LocalBundleAdjustment(pKF, pbStopFlag, pMap) (src/Optimizer.cc:586-853) from the assembled
    // graph on: the local keyframes' and fixed cameras' poses kfTcw (12 floats each, rows 0..2),
    // kfFixed (lFixedCameras and mnId == 0), kfSlot (each keyframe's row of mvKeysUn / mvuRight,
    // `cap` keypoints per row; mvuRight empty: monocular), the local points mpPos (3 floats
    // each), and per point (obsOff, CSR) its observations as (keyframe index obsKF, keypoint
    // index obsKP).  The covisibility walk stays with the caller and the stop flag is not
    // supported.  kfTcw and mpPos are updated in place as SetPose / SetWorldPos do; vToErase
    // gets one flag per observation; returns their number.  trace (optional, 4 ints): per
    // optimisation the LM iterations run and the linear solves tried; status (optional): the
    // ORBX_LOCAL_BA_STATUS_* bits.
    static int LocalBundleAdjustment(ORBmatcher& matcher, std::vector<float>& kfTcw, const std::vector<uint8_t>& kfFixed,
                                     const std::vector<int32_t>& kfSlot, std::vector<float>& mpPos,
                                     const std::vector<int32_t>& obsOff, const std::vector<int32_t>& obsKF,
                                     const std::vector<int32_t>& obsKP, const std::vector<orbx_keypoint>& mvKeysUn,
                                     const std::vector<float>& mvuRight, int cap,
                                     const std::vector<float>& mvInvLevelSigma2, float fx, float fy, float cx, float cy,
                                     float mbf, std::vector<uint8_t>& vToErase, int32_t* trace = nullptr,
                                     int* status = nullptr, std::vector<uint8_t>* level1 = nullptr) {
        const int32_t nkf = (int32_t)kfFixed.size(), npt = (int32_t)(mpPos.size() / 3), nobs = (int32_t)obsKF.size();
        if (cap <= 0 || kfTcw.size() != (size_t)nkf * 12 || kfSlot.size() != (size_t)nkf ||
            obsOff.size() != (size_t)npt + 1 || obsKP.size() != (size_t)nobs || mvKeysUn.size() % (size_t)cap ||
            (!mvuRight.empty() && mvuRight.size() != mvKeysUn.size()))
            throw std::runtime_error("LocalBundleAdjustment: array sizes differ");
        const int32_t kf_off[2] = {0, nkf}, pt_off[2] = {0, npt};
        std::vector<float> Tout(kfTcw.size()), Xout(mpPos.size());
        vToErase.assign((size_t)nobs, 0);
        if (level1) level1->assign((size_t)nobs, 0);
        int32_t n_erase = 0, st = 0;
        orbx_local_ba_batch q{};
        q.batch = 1;
        q.kf_off = kf_off;
        q.n_kf = nkf;
        q.kf_Tcw = kfTcw.data();
        q.kf_fixed = kfFixed.data();
        q.kf_slot = kfSlot.data();
        q.pt_off = pt_off;
        q.n_pt = npt;
        q.pt_pos = mpPos.data();
        q.obs_off = obsOff.data();
        q.n_obs = nobs;
        q.obs_kf = obsKF.data();
        q.obs_kp = obsKP.data();
        q.n_slots = (int)(mvKeysUn.size() / (size_t)cap);
        q.cap = cap;
        q.kps = mvKeysUn.data();
        q.u_right = mvuRight.empty() ? nullptr : mvuRight.data();
        q.inv_level_sigma2 = mvInvLevelSigma2.data();
        q.nlevels = (int)mvInvLevelSigma2.size();
        q.fx = fx;
        q.fy = fy;
        q.cx = cx;
        q.cy = cy;
        q.bf = mbf;
        q.kf_Tcw_opt = Tout.data();
        q.pt_pos_opt = Xout.data();
        q.erase = vToErase.data();
        q.level1 = level1 ? level1->data() : nullptr;
        q.n_erase = &n_erase;
        q.trace = trace;
        q.status = &st;
        check(orbx_local_bundle_adjustment(matcher.handle(), &q));
        kfTcw = Tout;
        mpPos = Xout;
        if (status) *status = st;
        return n_erase;
    }

    // BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)
    // (src/Optimizer.cc:41-281), which GlobalBundleAdjustemnt calls with the whole map, from the
    // assembled graph on: the tables of LocalBundleAdjustment above with the good keyframes and
    // points of the map, kfFixed = (mnId == 0).  The stop flag is not supported, and where the
    // results go (SetPose / SetWorldPos or mTcwGBA / mPosGBA, the nLoopKF switch) is the
    // caller's business: kfTcw (every keyframe, the fixed ones as their round trip through the
    // quaternion) and mpPos are updated in place; vbNotIncludedMP gets one flag per point (1: the
    // point has no edge and keeps its position).  trace (optional, 2 ints): the LM iterations
    // run and the linear solves tried; chi2 (optional, 2 doubles): initial and final.  Returns
    // the ORBX_GLOBAL_BA_STATUS_* bits.
    static int BundleAdjustment(ORBmatcher& matcher, std::vector<float>& kfTcw, const std::vector<uint8_t>& kfFixed,
                                const std::vector<int32_t>& kfSlot, std::vector<float>& mpPos,
                                const std::vector<int32_t>& obsOff, const std::vector<int32_t>& obsKF,
                                const std::vector<int32_t>& obsKP, const std::vector<orbx_keypoint>& mvKeysUn,
                                const std::vector<float>& mvuRight, int cap, const std::vector<float>& mvInvLevelSigma2,
                                float fx, float fy, float cx, float cy, float mbf, int nIterations = 5,
                                bool bRobust = true, std::vector<uint8_t>* vbNotIncludedMP = nullptr,
                                int32_t* trace = nullptr, double* chi2 = nullptr) {
        const int32_t nkf = (int32_t)kfFixed.size(), npt = (int32_t)(mpPos.size() / 3), nobs = (int32_t)obsKF.size();
        if (cap <= 0 || kfTcw.size() != (size_t)nkf * 12 || kfSlot.size() != (size_t)nkf ||
            obsOff.size() != (size_t)npt + 1 || obsKP.size() != (size_t)nobs || mvKeysUn.size() % (size_t)cap ||
            (!mvuRight.empty() && mvuRight.size() != mvKeysUn.size()))
            throw std::runtime_error("BundleAdjustment: array sizes differ");
        const int32_t kf_off[2] = {0, nkf}, pt_off[2] = {0, npt};
        std::vector<float> Tout(kfTcw.size()), Xout(mpPos.size());
        std::vector<uint8_t> included((size_t)npt + 1, 0);
        int32_t st = 0;
        orbx_global_ba_batch q{};
        check(orbx_global_ba_envelope(nkf, kfFixed.data(), npt, obsOff.data(), obsKF.data(), nobs, &q.max_env_blocks));
        q.batch = 1;
        q.kf_off = kf_off;
        q.n_kf = nkf;
        q.kf_Tcw = kfTcw.data();
        q.kf_fixed = kfFixed.data();
        q.kf_slot = kfSlot.data();
        q.pt_off = pt_off;
        q.n_pt = npt;
        q.pt_pos = mpPos.data();
        q.obs_off = obsOff.data();
        q.n_obs = nobs;
        q.obs_kf = obsKF.data();
        q.obs_kp = obsKP.data();
        q.n_slots = (int)(mvKeysUn.size() / (size_t)cap);
        q.cap = cap;
        q.kps = mvKeysUn.data();
        q.u_right = mvuRight.empty() ? nullptr : mvuRight.data();
        q.inv_level_sigma2 = mvInvLevelSigma2.data();
        q.nlevels = (int)mvInvLevelSigma2.size();
        q.fx = fx;
        q.fy = fy;
        q.cx = cx;
        q.cy = cy;
        q.bf = mbf;
        q.iterations = nIterations;
        q.robust = bRobust ? 1 : 0;
        q.kf_Tcw_opt = Tout.data();
        q.pt_pos_opt = Xout.data();
        q.pt_included = included.data();
        q.trace = trace;
        q.chi2 = chi2;
        q.status = &st;
        check(orbx_global_bundle_adjustment(matcher.handle(), &q));
        kfTcw = Tout;
        mpPos = Xout;
        if (vbNotIncludedMP) {
            vbNotIncludedMP->resize((size_t)npt);
            for (int32_t j = 0; j < npt; j++) (*vbNotIncludedMP)[(size_t)j] = included[(size_t)j] ? 0 : 1;
        }
        return st;
    }

    // OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
    // LoopConnections, bFixScale) (src/Optimizer.cc:873-1150) from the assembled graph on: the
    // good keyframes' non-corrected poses kfTcw (12 floats each, rows 0..2, ascending mnId),
    // kfCorr (the keyframe's row of corrS, the CorrectedSim3 as q xyzw, t, s; -1: none), the
    // row loopKF of pLoopKF, the edges (edgeV: vertex 0 and vertex 1 of each; edgeKind: 0 the
    // LoopConnections edges, 1 the others) in g2o's insertion order, the map points mpPos (3
    // floats each) and mpRef (the row of mnCorrectedReference or of the reference keyframe).
    // kfTcw and mpPos are updated in place as SetPose / SetWorldPos do.  Scw (optional): the
    // optimised Sim3 of every keyframe, 8 doubles each; trace (optional, 2 ints): the LM
    // iterations run and the linear solves tried; chi2 (optional, 2 doubles): initial and
    // final.  Returns the ORBX_ESSENTIAL_GRAPH_STATUS_* bits.
    static int OptimizeEssentialGraph(ORBmatcher& matcher, std::vector<float>& kfTcw, const std::vector<int32_t>& kfCorr,
                                      const std::vector<double>& corrS, int loopKF, const std::vector<int32_t>& edgeV,
                                      const std::vector<int32_t>& edgeKind, std::vector<float>& mpPos,
                                      const std::vector<int32_t>& mpRef, bool bFixScale,
                                      std::vector<double>* Scw = nullptr, int32_t* trace = nullptr,
                                      double* chi2 = nullptr, int iterations = 0) {
        const int32_t nkf = (int32_t)kfCorr.size(), ne = (int32_t)edgeKind.size(), npt = (int32_t)mpRef.size();
        if (kfTcw.size() != (size_t)nkf * 12 || corrS.size() % 8 || edgeV.size() != (size_t)ne * 2 ||
            mpPos.size() != (size_t)npt * 3)
            throw std::runtime_error("OptimizeEssentialGraph: array sizes differ");
        const int32_t kf_off[2] = {0, nkf}, edge_off[2] = {0, ne}, pt_off[2] = {0, npt}, loop = loopKF;
        std::vector<float> Tout(kfTcw.size()), Xout(mpPos.size());
        if (Scw) Scw->assign((size_t)nkf * 8, 0.0);
        int32_t st = 0;
        orbx_essential_graph_batch q{};
        check(orbx_essential_graph_envelope(nkf, loopKF, edgeV.data(), ne, &q.max_env_blocks));
        q.batch = 1;
        q.kf_off = kf_off;
        q.n_kf = nkf;
        q.kf_Tcw = kfTcw.data();
        q.kf_corr = kfCorr.data();
        q.corr_S = corrS.data();
        q.n_corr = (int)(corrS.size() / 8);
        q.loop_kf = &loop;
        q.edge_off = edge_off;
        q.n_edges = ne;
        q.edge_v = edgeV.data();
        q.edge_kind = edgeKind.data();
        q.pt_off = pt_off;
        q.n_pt = npt;
        q.pt_pos = mpPos.data();
        q.pt_ref = mpRef.data();
        q.fix_scale = bFixScale ? 1 : 0;
        q.iterations = iterations;
        q.kf_Tcw_opt = Tout.data();
        q.pt_pos_opt = Xout.data();
        q.Scw_opt = Scw ? Scw->data() : nullptr;
        q.trace = trace;
        q.chi2 = chi2;
        q.status = &st;
        check(orbx_optimize_essential_graph(matcher.handle(), &q));
        kfTcw = Tout;
        mpPos = Xout;
        return st;
    }
};

// LocalMapping::CreateNewMapPoints' triangulation and tests (src/LocalMapping.cc:307-501) for one
// keyframe pair on host arrays (orbx_triangulate_pairs).
class LocalMapping {
public:
    // One KeyFrame as the triangulation reads it: mvKeysUn, mvKeys (empty: mvKeysUn), mvuRight
    // (empty: monocular), mvDepth (empty: mbf / (mvKeys.x - mvuRight) in float), mTcw rows 0..2.
    struct KeyFrameGeom {
        std::vector<orbx_keypoint> mvKeysUn, mvKeys;
        std::vector<float> mvuRight, mvDepth;
        float mTcw[12];
    };
    // The new MapPoints of one pair row: per matched pair the reason (0 = accepted) and the branch
    // taken, the point's mWorldPos / mNormalVector / mfMaxDistance / mfMinDistance, and the accepted
    // slots in the order the reference creates the points in.
    struct NewMapPoints {
        std::vector<uint8_t> reason, method;
        std::vector<float> pos, normal, maxDistance, minDistance;
        std::vector<int32_t> newIdx;
    };
    // vMatchedIndices: (idx1, idx2) per matched pair, as SearchForTriangulation returns them.  cam:
    // fx fy cx cy and the level tables; mb / mbf of KF1.  Returns nnew.
    static int TriangulatePairs(ORBmatcher& matcher, const KeyFrameGeom& KF1, const KeyFrameGeom& KF2,
                                const orbx_frame_view& cam, const std::vector<int32_t>& vMatchedIndices, float mb,
                                float mbf, NewMapPoints& out) {
        const int k = (int)(vMatchedIndices.size() / 2);
        const int32_t n1 = (int32_t)KF1.mvKeysUn.size(), n2 = (int32_t)KF2.mvKeysUn.size();
        auto sized = [](const KeyFrameGeom& K, size_t n) {
            return (K.mvKeys.empty() || K.mvKeys.size() == n) && (K.mvuRight.empty() || K.mvuRight.size() == n) &&
                   (K.mvDepth.empty() || K.mvDepth.size() == n);
        };
        if (!sized(KF1, (size_t)n1) || !sized(KF2, (size_t)n2))
            throw std::runtime_error("TriangulatePairs: array sizes differ");
        const orbx_keypoint kp0{};  // the call takes no null mvKeysUn: an empty one gets one spare element
        auto rec = [&kp0](const KeyFrameGeom& K, const int32_t* n) {
            orbx_keyframe_geom_device g{};
            g.keys_un = K.mvKeysUn.empty() ? &kp0 : K.mvKeysUn.data();
            g.keys = K.mvKeys.empty() ? nullptr : K.mvKeys.data();
            g.u_right = K.mvuRight.empty() ? nullptr : K.mvuRight.data();
            g.depth = K.mvDepth.empty() ? nullptr : K.mvDepth.data();
            g.n = n;
            for (int i = 0; i < 12; i++) g.Tcw[i] = K.mTcw[i];
            return g;
        };
        const orbx_keyframe_geom_device g1 = rec(KF1, &n1), g2 = rec(KF2, &n2);
        const size_t c = (size_t)(k > 0 ? k : 1);
        out.reason.assign(c, 0);
        out.method.assign(c, 0);
        out.pos.assign(3 * c, 0.0f);
        out.normal.assign(3 * c, 0.0f);
        out.maxDistance.assign(c, 0.0f);
        out.minDistance.assign(c, 0.0f);
        out.newIdx.assign(c, 0);
        int32_t nnew = 0;
        const orbx_new_mappoints o{out.reason.data(), out.method.data(), out.pos.data(), out.normal.data(),
                                   out.maxDistance.data(), out.minDistance.data(), &nnew, out.newIdx.data()};
        const int32_t none[2] = {-1, -1};
        check(orbx_triangulate_pairs(matcher.handle(), &g1, &g2, &cam, k, k > 0 ? vMatchedIndices.data() : none, mb, mbf,
                                     &o));
        out.reason.resize((size_t)k);
        out.method.resize((size_t)k);
        out.pos.resize(3 * (size_t)k);
        out.normal.resize(3 * (size_t)k);
        out.maxDistance.resize((size_t)k);
        out.minDistance.resize((size_t)k);
        out.newIdx.resize((size_t)nnew);
        return nnew;
    }
};

// DBoW2::BowVector (BowVector.h:59-62): word id -> value, ascending.
typedef std::map<int32_t, double> BowVector;

inline void BowArrays(const BowVector& v, std::vector<int32_t>& words, std::vector<double>& values) {
    words.clear();
    values.clear();
    for (const auto& e : v) {
        words.push_back(e.first);
        values.push_back(e.second);
    }
}

// L1Scoring::score(v1, v2) (DBoW2 ScoringObject.cpp:23-68); host only.
inline double BowScore(const BowVector& v1, const BowVector& v2) {
    std::vector<int32_t> w1, w2;
    std::vector<double> a1, a2;
    BowArrays(v1, w1, a1);
    BowArrays(v2, w2, a2);
    double s = 0.0;
    check(orbx_bow_score(w1.data(), a1.data(), (int)w1.size(), w2.data(), a2.data(), (int)w2.size(), &s));
    return s;
}

// ORBVocabulary (include/ORBVocabulary.h = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>):
// loadFromTextFile, size, transform to a BowVector, score (L1_NORM only).
class ORBVocabulary {
public:
    explicit ORBVocabulary(int device = 0) : device_(device) {}
    ~ORBVocabulary() { orbx_vocabulary_destroy(h_); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    bool loadFromTextFile(const std::string& filename) {
        orbx_vocabulary_destroy(h_);
        h_ = nullptr;
        const int rc = orbx_vocabulary_load_text_file(filename.c_str(), device_, &h_);
        if (rc == ORBX_ERR_ARG) return false;
        check(rc);
        return true;
    }
    unsigned int size() const {
        int n = 0;
        check(orbx_vocabulary_info(h_, nullptr, nullptr, nullptr, nullptr, nullptr, &n));
        return (unsigned)n;
    }
    // transform(features, BowVector&, FeatureVector&, levelsup): the BowVector part
    void transform(const uint8_t* descriptors, int n, BowVector& v, int levelsup = 4) {
        std::vector<int32_t> bw((size_t)n + 1), fn((size_t)n + 1), fo((size_t)n + 2), fi((size_t)n + 1);
        std::vector<double> bv((size_t)n + 1);
        int nb = 0, nf = 0;
        check(orbx_vocabulary_transform(h_, descriptors, n, levelsup, bw.data(), bv.data(), &nb, fn.data(), fo.data(),
                                        fi.data(), &nf));
        v.clear();
        for (int i = 0; i < nb; i++) v.emplace_hint(v.end(), bw[i], bv[i]);
    }
    // score(v1, v2), TemplatedVocabulary.h:1198-1203
    double score(const BowVector& v1, const BowVector& v2) const {
        int scoring = 0;
        check(orbx_vocabulary_info(h_, nullptr, nullptr, &scoring, nullptr, nullptr, nullptr));
        if (scoring != 0) throw Error(ORBX_ERR_UNSUPPORTED, "orbx: only L1_NORM scoring is built");
        return BowScore(v1, v2);
    }
    orbx_vocabulary* handle() const { return h_; }

private:
    orbx_vocabulary* h_ = nullptr;
    int device_;
};

// KeyFrameDatabase (include/KeyFrameDatabase.h:40-92, src/KeyFrameDatabase.cc:31-307).  A
// KeyFrame* is a caller-chosen id in [0, maxKeyFrames); add() takes the keyframe's mBowVec,
// SetBestCovisibility its GetBestCovisibilityKeyFrames(10), DetectLoopCandidates its
// GetConnectedKeyFrames().
class KeyFrameDatabase {
public:
    explicit KeyFrameDatabase(const ORBVocabulary& voc, int maxKeyFrames = 4096, int maxWords = 2048)
        : max_(maxKeyFrames) {
        check(orbx_kfdb_create(voc.handle(), maxKeyFrames, maxWords, &h_));
    }
    ~KeyFrameDatabase() { orbx_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    // add(pKF): device BowVectors in the orbx_vocabulary_transform_batch_device layout
    void add(const std::vector<int32_t>& ids, const int32_t* d_bow_word, const double* d_bow_value,
             const int32_t* d_nbow, int src_cap, void* stream = nullptr) {
        check(orbx_kfdb_add_batch_device(h_, (int)ids.size(), ids.data(), d_bow_word, d_bow_value, d_nbow, src_cap,
                                         stream));
    }
    // add(pKF) from a host BowVector
    void add(int id, const BowVector& bowVec) {
        std::vector<int32_t> w;
        std::vector<double> v;
        BowArrays(bowVec, w, v);
        check(orbx_kfdb_add(h_, id, w.data(), v.data(), (int)w.size()));
    }
    void erase(int id) { check(orbx_kfdb_erase(h_, id)); }
    void clear() { check(orbx_kfdb_clear(h_)); }
    void SetBestCovisibility(int id, const std::vector<int32_t>& best) {
        check(orbx_kfdb_set_covisibility(h_, id, best.data(), (int)best.size()));
    }
    // vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore)
    std::vector<int32_t> DetectLoopCandidates(const BowVector& bowVec, const std::set<int32_t>& connected,
                                              float minScore) {
        std::vector<int32_t> w, c(connected.begin(), connected.end()), out((size_t)max_);
        std::vector<double> v;
        BowArrays(bowVec, w, v);
        int n = 0;
        check(orbx_kfdb_detect_loop_candidates(h_, w.data(), v.data(), (int)w.size(), c.data(), (int)c.size(), minScore,
                                               out.data(), max_, &n));
        out.resize((size_t)n);
        return out;
    }
    // vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)
    std::vector<int32_t> DetectRelocalizationCandidates(const BowVector& bowVec) {
        std::vector<int32_t> w, out((size_t)max_);
        std::vector<double> v;
        BowArrays(bowVec, w, v);
        int n = 0;
        check(orbx_kfdb_detect_relocalization_candidates(h_, w.data(), v.data(), (int)w.size(), out.data(), max_, &n));
        out.resize((size_t)n);
        return out;
    }
    orbx_kfdb* handle() { return h_; }

private:
    orbx_kfdb* h_ = nullptr;
    int max_;
};

// Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc:37-534) on the arrays the adapter
// extracts: vpKeyFrameMP1 / vpMatched12 as MapPoint ids into mpPos
// (GetWorldPos(), 3 floats per id; -1 for NULL, isBad() and GetIndexInKeyFrame() < 0), the
// octaves of kp1 / kp2 per slot, the two keyframes' poses (rows 0..2, 12 floats),
// mvLevelSigma2 and fx fy cx cy of each.  draws: 3 per iteration (empty: the reference's, from
// rand(), taken when SetRansacParameters runs).  Runs on the matcher's handle and stream; the
// matcher must outlive the solver.  iterate returns T12 (16 floats, row-major; empty: the
// reference's empty Mat).
class Sim3Solver {
public:
    Sim3Solver(ORBmatcher& matcher, const std::vector<int32_t>& vpKeyFrameMP1, const std::vector<int32_t>& vpMatched12,
               const std::vector<int32_t>& octaves1, const std::vector<int32_t>& octaves2,
               const std::vector<float>& mpPos, const float* Tcw1, const float* Tcw2,
               const std::vector<float>& mvLevelSigma2, const float* K1, const float* K2, bool bFixScale,
               const std::vector<int32_t>& draws = {})
        : m_(matcher.handle()), mp1_(vpKeyFrameMP1), mp2_(vpMatched12), oct1_(octaves1), oct2_(octaves2), pos_(mpPos),
          sig_(mvLevelSigma2), draws_(draws), fix_(bFixScale) {
        mN1 = (int)mp2_.size();
        if (mp1_.size() < mp2_.size() || oct1_.size() < mp2_.size() || oct2_.size() < mp2_.size())
            throw Error(ORBX_ERR_ARG, "Sim3Solver: one MapPoint and two octaves per slot of vpMatched12");
        for (int i = 0; i < 12; i++) T1_[i] = Tcw1[i], T2_[i] = Tcw2[i];
        for (int i = 0; i < 4; i++) K1_[i] = K1[i], K2_[i] = K2[i];
        SetRansacParameters();  // cc:128
    }
    ~Sim3Solver() { orbx_sim3_destroy(h_); }
    Sim3Solver(const Sim3Solver&) = delete;
    Sim3Solver& operator=(const Sim3Solver&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        if (!h_ || maxIterations > maxIts_) {
            orbx_sim3_destroy(h_);
            h_ = nullptr;
            check(orbx_sim3_create(m_, 1, mN1 > 0 ? mN1 : 1, maxIterations, &h_));
            maxIts_ = maxIterations;
        }
        std::vector<int32_t> d(draws_);
        if (d.empty()) {
            int N = 0;
            const int n_mp = (int)(pos_.size() / 3);
            for (int i = 0; i < mN1; i++)
                N += mp1_[i] >= 0 && mp1_[i] < n_mp && mp2_[i] >= 0 && mp2_[i] < n_mp;
            d.resize((size_t)maxIterations * 3);
            check(orbx_sim3_draws(d.data(), N, maxIterations));
        }
        if (d.size() < (size_t)maxIterations * 3) throw Error(ORBX_ERR_ARG, "Sim3Solver: fewer draws than iterations");
        orbx_sim3_batch in{};
        const int32_t n1 = mN1;
        in.batch = 1;
        in.cap = mN1 > 0 ? mN1 : 1;
        in.n1 = &n1;
        const int32_t none = -1;  // mN1 == 0: the arrays are not read
        in.mp1 = mN1 ? mp1_.data() : &none;
        in.mp2 = mN1 ? mp2_.data() : &none;
        in.oct1 = mN1 ? oct1_.data() : &none;
        in.oct2 = mN1 ? oct2_.data() : &none;
        in.n_mp = (int)(pos_.size() / 3);
        in.mp_pos = pos_.data();
        in.Tcw1 = T1_;
        in.Tcw2 = T2_;
        in.level_sigma2 = sig_.data();
        in.nlevels = (int)sig_.size();
        in.K1 = K1_;
        in.K2 = K2_;
        in.fix_scale = fix_ ? 1 : 0;
        in.probability = probability;
        in.min_inliers = minInliers;
        in.max_iterations = maxIterations;
        in.draws = d.data();
        check(orbx_sim3_set(h_, &in));
        its_ = maxIterations;
    }

    std::vector<float> iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        std::vector<uint8_t> inl((size_t)(mN1 > 0 ? mN1 : 1), 0);
        std::vector<float> T((size_t)16);
        int32_t found = 0, no_more = 0, n = 0;
        orbx_sim3_result out{};
        out.found = &found;
        out.no_more = &no_more;
        out.n_inliers = &n;
        out.inliers = inl.data();
        out.T12 = T.data();
        out.best_R = R_;
        out.best_t = t_;
        out.best_s = &s_;
        out.best_inliers = &bestInliers;
        out.best_iteration = &bestIteration;
        out.iterations = &iterations;
        out.n_pairs = &N;
        out.status = &status;
        check(orbx_sim3_iterate(h_, nIterations, &out));
        bNoMore = no_more != 0;
        nInliers = n;
        vbInliers.assign((size_t)mN1, false);
        for (int i = 0; i < mN1; i++) vbInliers[(size_t)i] = inl[(size_t)i] != 0;
        if (!found) T.clear();
        return T;
    }
    std::vector<float> find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(its_, bFlag, vbInliers12, nInliers);  // cc:277-281
    }
    std::vector<float> GetEstimatedRotation() const { return std::vector<float>(R_, R_ + 9); }
    std::vector<float> GetEstimatedTranslation() const { return std::vector<float>(t_, t_ + 3); }
    float GetEstimatedScale() const { return s_; }
    orbx_sim3* handle() { return h_; }

    // after an iterate: mnBestInliers, the absolute iteration holding the best state (-1: none),
    // mnIterations, N and the ORBX_SIM3_STATUS_* bits
    int32_t bestInliers = 0, bestIteration = -1, iterations = 0, N = 0, status = 0;

private:
    orbx_matcher* m_;
    orbx_sim3* h_ = nullptr;
    std::vector<int32_t> mp1_, mp2_, oct1_, oct2_;
    std::vector<float> pos_, sig_;
    std::vector<int32_t> draws_;
    bool fix_;
    int mN1 = 0, maxIts_ = 0, its_ = 0;
    float T1_[12], T2_[12], K1_[4], K2_[4];
    float R_[9] = {}, t_[3] = {}, s_ = 0.0f;
};

// PnPsolver (include/PnPsolver.h, src/PnPsolver.cc:80-1345) on the arrays the adapter extracts
// (INTEGRATION.md §4g): F.mvKeysUn, vpMapPointMatches as MapPoint ids into mpPos (GetWorldPos(),
// 3 floats per id; -1 for NULL and isBad()), F.mvLevelSigma2 and fx fy cx cy.  draws: 4 per
// iteration (empty: the reference's, from rand(), taken when SetRansacParameters runs: twice
// maxIterations of them, since a call after the first runs beyond the cap, cc:226).  Runs on
// the matcher's handle and stream; the matcher must outlive the solver.  iterate returns Tcw
// (16 floats, row-major; empty: the reference's empty Mat).
class PnPsolver {
public:
    PnPsolver(ORBmatcher& matcher, const std::vector<orbx_keypoint>& mvKeysUn,
              const std::vector<int32_t>& vpMapPointMatches, const std::vector<float>& mpPos,
              const std::vector<float>& mvLevelSigma2, const float* K, const std::vector<int32_t>& draws = {})
        : m_(matcher.handle()), keys_(mvKeysUn), mp_(vpMapPointMatches), pos_(mpPos), sig_(mvLevelSigma2),
          draws_(draws) {
        n_ = (int)mp_.size();
        if (keys_.size() < mp_.size()) throw Error(ORBX_ERR_ARG, "PnPsolver: one keypoint per slot of vpMapPointMatches");
        for (int i = 0; i < 4; i++) K_[i] = K[i];
        try {
            SetRansacParameters();  // cc:127
        } catch (...) {  // no destructor runs for a constructor that throws
            orbx_pnp_destroy(h_);
            throw;
        }
    }
    ~PnPsolver() { orbx_pnp_destroy(h_); }
    PnPsolver(const PnPsolver&) = delete;
    PnPsolver& operator=(const PnPsolver&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4f, float th2 = 5.991f) {
        std::vector<int32_t> d(draws_);
        if (d.empty()) {
            int N = 0;
            const int n_mp = (int)(pos_.size() / 3);
            for (int i = 0; i < n_; i++) N += mp_[i] >= 0 && mp_[i] < n_mp;
            d.resize((size_t)maxIterations * 8);
            check(orbx_pnp_draws(d.data(), N, 2 * maxIterations));
        }
        const int nDraws = (int)(d.size() / 4);
        if (!h_ || nDraws > maxDraws_) {
            orbx_pnp_destroy(h_);
            h_ = nullptr;
            check(orbx_pnp_create(m_, 1, n_ > 0 ? n_ : 1, nDraws > 0 ? nDraws : 1, &h_));
            maxDraws_ = nDraws;
        }
        orbx_pnp_batch in{};
        const int32_t n = n_;
        const int32_t none = -1;  // n == 0: the arrays are not read
        const orbx_keypoint nokey{};
        in.batch = 1;
        in.cap = n_ > 0 ? n_ : 1;
        in.kps = n_ ? keys_.data() : &nokey;
        in.n = &n;
        in.matches = n_ ? mp_.data() : &none;
        in.n_mp = (int)(pos_.size() / 3);
        in.mp_pos = pos_.data();
        in.level_sigma2 = sig_.data();
        in.nlevels = (int)sig_.size();
        in.fx = K_[0];
        in.fy = K_[1];
        in.cx = K_[2];
        in.cy = K_[3];
        in.probability = probability;
        in.min_inliers = minInliers;
        in.max_iterations = maxIterations;
        in.min_set = minSet;
        in.epsilon = epsilon;
        in.th2 = th2;
        in.draws = d.data();
        in.n_draws = nDraws;
        check(orbx_pnp_set(h_, &in));
        its_ = maxIterations;
    }

    std::vector<float> iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        std::vector<uint8_t> inl((size_t)(n_ > 0 ? n_ : 1), 0);
        frameMP.assign((size_t)(n_ > 0 ? n_ : 1), -1);
        float T[12] = {};
        int32_t found = 0, no_more = 0, n = 0;
        orbx_pnp_result out{};
        out.found = &found;
        out.no_more = &no_more;
        out.n_inliers = &n;
        out.inliers = inl.data();
        out.Tcw = T;
        out.frame_mp = frameMP.data();
        out.best_Tcw = bestTcw;
        out.best_inliers = &bestInliers;
        out.best_iteration = &bestIteration;
        out.refined = &refined;
        out.iterations = &iterations;
        out.n_corr = &N;
        out.min_inliers_used = &minInliersUsed;
        out.max_its_used = &maxItsUsed;
        out.status = &status;
        check(orbx_pnp_iterate(h_, nIterations, &out));
        frameMP.resize((size_t)n_);
        bNoMore = no_more != 0;
        nInliers = n;
        vbInliers.assign((size_t)n_, false);
        for (int i = 0; i < n_; i++) vbInliers[(size_t)i] = inl[(size_t)i] != 0;
        std::vector<float> Tcw;
        if (found) {
            Tcw.assign(T, T + 12);
            Tcw.insert(Tcw.end(), {0.0f, 0.0f, 0.0f, 1.0f});
        }
        return Tcw;
    }
    std::vector<float> find(std::vector<bool>& vbInliers, int& nInliers) {
        bool bFlag;
        return iterate(its_, bFlag, vbInliers, nInliers);  // cc:193-197
    }
    orbx_pnp* handle() { return h_; }

    // after an iterate: mBestTcw (rows 0..2), mnBestInliers, the absolute iteration holding the
    // best state (-1: none), whether the returned pose came from Refine(), mnIterations, N, the
    // adjusted mRansacMinInliers / mRansacMaxIts, the ORBX_PNP_STATUS_* bits, and the frame's
    // MapPoint ids with the outliers cleared (Tracking.cc:1600-1612)
    float bestTcw[12] = {};
    int32_t bestInliers = 0, bestIteration = -1, refined = 0, iterations = 0, N = 0, minInliersUsed = 0, maxItsUsed = 0,
            status = 0;
    std::vector<int32_t> frameMP;

private:
    orbx_matcher* m_;
    orbx_pnp* h_ = nullptr;
    std::vector<orbx_keypoint> keys_;
    std::vector<int32_t> mp_;
    std::vector<float> pos_, sig_;
    std::vector<int32_t> draws_;
    int n_ = 0, maxDraws_ = 0, its_ = 0;
    float K_[4];
};

// Initializer (include/Initializer.h, src/Initializer.cc:64-1415) on the arrays the adapter
// extracts: mvKeysUn of the reference frame at construction (Initializer(ReferenceFrame, sigma,
// iterations), cc:43-56, with K as fx fy cx cy), mvKeysUn of the current frame and vMatches12 per
// call.  sets: 8 per iteration (empty: the reference's, from srand(0) and rand()).  Runs on the
// matcher's handle and stream; the matcher must outlive it.
class Initializer {
public:
    Initializer(ORBmatcher& matcher, const std::vector<orbx_keypoint>& mvKeys1, const float* K, float sigma = 1.0f,
                int iterations = 200)
        : m_(matcher.handle()), keys1_(mvKeys1), sigma_(sigma), its_(iterations) {
        for (int i = 0; i < 4; i++) K_[i] = K[i];
    }
    ~Initializer() { orbx_initializer_destroy(h_); }
    Initializer(const Initializer&) = delete;
    Initializer& operator=(const Initializer&) = delete;

    // Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) (cc:64-165): R21 (9
    // floats, row-major) and t21 (3) are empty when it returns false; vP3D holds 3 floats per
    // keypoint of the reference frame.
    bool Initialize(const std::vector<orbx_keypoint>& mvKeys2, const std::vector<int32_t>& vMatches12,
                    std::vector<float>& R21, std::vector<float>& t21, std::vector<float>& vP3D,
                    std::vector<bool>& vbTriangulated, const std::vector<int32_t>& sets = {}) {
        const int32_t n1 = (int32_t)keys1_.size(), n2 = (int32_t)mvKeys2.size();
        if (vMatches12.size() != keys1_.size())
            throw Error(ORBX_ERR_ARG, "Initializer: one vMatches12 entry per keypoint of the reference frame");
        const int kcap = std::max(1, std::max(n1, n2));
        if (!h_ || kcap > kcap_) {
            orbx_initializer_destroy(h_);
            h_ = nullptr;
            check(orbx_initializer_create(m_, 1, kcap, its_, &h_));
            kcap_ = kcap;
        }
        std::vector<int32_t> s(sets);
        if (s.empty()) {
            int N = 0;
            for (int32_t v : vMatches12) N += v >= 0 && v < n2;
            s.resize((size_t)its_ * 8);
            check(orbx_initializer_sets(s.data(), N, its_));
        }
        if (s.size() < (size_t)its_ * 8) throw Error(ORBX_ERR_ARG, "Initializer: fewer sets than iterations");
        const orbx_keypoint none{};  // an empty frame: the array is not read
        orbx_initializer_batch in{};
        in.batch = 1;
        in.kcap = kcap;
        in.n1 = &n1;
        in.n2 = &n2;
        in.keys1 = n1 ? keys1_.data() : &none;
        in.keys2 = n2 ? mvKeys2.data() : &none;
        const int32_t no_match = -1;
        in.matches12 = n1 ? vMatches12.data() : &no_match;
        in.K = K_;
        in.sigma = sigma_;
        in.max_iterations = its_;
        in.sets = s.data();
        std::vector<uint8_t> tri((size_t)kcap, 0);
        inliersH.assign((size_t)kcap, 0);
        inliersF.assign((size_t)kcap, 0);
        R21.assign(9, 0.0f);
        t21.assign(3, 0.0f);
        vP3D.assign((size_t)kcap * 3, 0.0f);
        int32_t ok = 0;
        orbx_initializer_result out{};
        out.ok = &ok;
        out.model = &model;
        out.n_matches = &N;
        out.SH = &SH;
        out.SF = &SF;
        out.RH = &RH;
        out.best_it_H = &bestIterationH;
        out.best_it_F = &bestIterationF;
        out.H21 = H21;
        out.F21 = F21;
        out.inliers_H = inliersH.data();
        out.inliers_F = inliersF.data();
        out.n_inliers_H = &nInliersH;
        out.n_inliers_F = &nInliersF;
        out.R21 = R21.data();
        out.t21 = t21.data();
        out.p3d = vP3D.data();
        out.triangulated = tri.data();
        out.best_good = &bestGood;
        out.second_good = &secondGood;
        out.n_similar = &nSimilar;
        out.parallax = &parallax;
        out.status = &status;
        check(orbx_initializer_initialize(h_, &in, &out));
        vP3D.resize((size_t)n1 * 3);
        inliersH.resize((size_t)n1);
        inliersF.resize((size_t)n1);
        vbTriangulated.assign((size_t)n1, false);
        for (int i = 0; i < n1; i++) vbTriangulated[(size_t)i] = tri[(size_t)i] != 0;
        if (!ok) {
            R21.clear();
            t21.clear();
        }
        return ok != 0;
    }
    orbx_initializer* handle() { return h_; }

    // after an Initialize: the model that was reconstructed (0 = H, 1 = F), N, the scores, the
    // best iterations (-1: none) and matrices, the inlier flags per keypoint of the reference
    // frame, ReconstructH / F's counts, the chosen hypothesis's parallax, the ORBX_INIT_STATUS_* bits
    int32_t model = 1, N = 0, bestIterationH = -1, bestIterationF = -1, nInliersH = 0, nInliersF = 0, bestGood = 0,
            secondGood = 0, nSimilar = 0, status = 0;
    float SH = 0.0f, SF = 0.0f, RH = 0.0f, parallax = 0.0f, H21[9] = {}, F21[9] = {};
    std::vector<uint8_t> inliersH, inliersF;

private:
    orbx_matcher* m_;
    orbx_initializer* h_ = nullptr;
    std::vector<orbx_keypoint> keys1_;
    float K_[4], sigma_;
    int its_, kcap_ = 0;
};

}  // namespace orbx
