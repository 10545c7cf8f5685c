// cs_patchmatch.h -- class CSPatchMatch with the reference's public interface (CSPM/cs_patchmatch.h:17-68).
#pragma once
#include "../../include/cspm.h"
#include <utility>

#include "commfunc.h"
#include "plane.h"
#include "plane_cost/i_plane_cost.h"

#define WMF_GAMMA 10.0

class CSPatchMatch {
 public:
  CSPatchMatch(const Mat &l_img, const Mat &r_img, const int &max_dis, const int &dis_scale);
  // RAW photographs of a calibrated rig (an addition; include/cspm.h "rectification"): the pair is rectified on the device (RectifyPair)
  // and the object is the one the constructor above makes of the result; rect comes from cspm_rectify_compute.  The plane cost it runs
  // on must see the same rectified pair: a device cost built from the raw pair through a DeviceSlot with SetRectification does.
  CSPatchMatch(const Mat &l_raw, const Mat &r_raw, const cspm_rig &rig, const cspm_rectification &rect, const int &max_dis, const int &dis_scale);
  ~CSPatchMatch();
  // init, iter_num x (spatial, view, refinement), PlaneToDisp, optional PostProcessing (cs_patchmatch.cc:51-109).
  // A device cost (PreSSPC / PreCSPC / GrdPC / CSPC of this host layer) runs the whole loop on its GPU.  Any other IPlaneCost
  // (a plugin: i_plane_cost.h:28-33) is priced through its GetPlaneCost, candidate batch by candidate batch, while the plane
  // field, the random streams and the accept rules stay on the device (PatchMatchForeign).
  void PatchMatch(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  Mat &dis(const RefView &view) { return dis_[view]; }
  // PatchMatch in two halves for callers that overlap their own work (file decoding, the previous pair's encoding) with the GPU:
  // Begin enqueues the whole loop on the cost object's stream and returns (a device cost; a foreign IPlaneCost runs to completion here),
  // End waits for it and fills dis() -- PlaneToDisp, or PostProcessing when use_pp.  PatchMatch == Begin + End.
  void PatchMatchBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  void PatchMatchEnd();
  // local stereo instead of PatchMatch (an addition): cost aggregation with ca_method (CSPM_CA_BOX / GF / BF) over one of this
  // library's PreSSPC / PreCSPC costs, then cross-scale winner-take-all of fronto-parallel planes (include/cspm.h
  // cspm_local_stereo); dis(), planes(), disparity() and use_pp as after PatchMatch.  Begin / End as above (End = PatchMatchEnd).
  void LocalStereo(const int &ca_method, const IPlaneCost *plane_cost, const bool &use_pp);
  void LocalStereoBegin(const int &ca_method, const IPlaneCost *plane_cost, const bool &use_pp);
  // slanted planes fitted to the disparity maps of the plane field in the device context of plane_cost (an addition; include/cspm.h
  // cspm_fit_planes) -- after LocalStereo(Begin), whose field is fronto-parallel, or any run.  merge = false: every plane is replaced
  // (PatchMatchFrom re-scores); merge = true: a fitted plane wins only where it costs less.  Enqueued on the cost object's stream: it
  // may follow a ...Begin on the same cost object and be followed by PatchMatchFromBegin / PatchMatchKeepBegin.  One of this
  // library's device costs only: a foreign IPlaneCost throws.
  void FitPlanes(const IPlaneCost *plane_cost, const cspm_fit_params &params, const bool &merge);
  // one robustly fitted plane per superpixel of the plane field in the device context of plane_cost (an addition; include/cspm.h
  // cspm_segment_planes), offered to every pixel of the segment.  merge = false: the planes of fitted segments replace the stored ones
  // (PatchMatchFrom re-scores); merge = true: a segment's plane wins only where it costs less.  Enqueued on the cost object's stream
  // like FitPlanes: it may follow any ...Begin on the same cost object and be followed by PatchMatchFromBegin.  One of this library's
  // device costs only: a foreign IPlaneCost throws.
  void SegmentPlanes(const IPlaneCost *plane_cost, const cspm_seg_params &params, const bool &merge);
  // warm start (an addition): iter_num PatchMatch iterations from the plane field already in the device context of plane_cost --
  // after LocalStereo, a previous pair's run, or the planes given to SetPlanes -- instead of InitRandomPlane.  The field is re-scored
  // under plane_cost first (include/cspm.h cspm_patchmatch_warm).  Begin may follow a LocalStereoBegin on the same cost object
  // without its End: the run is enqueued behind it.  One of this library's device costs only: a foreign IPlaneCost throws.
  void PatchMatchFrom(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  void PatchMatchFromBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  // the starting planes of a view for the next PatchMatchFrom (a previous frame's planes(), for example): wid x hei, row-major.
  // Kept here and written into the cost object's context when PatchMatchFromBegin runs.
  void SetPlanes(const RefView &view, const std::vector<Plane> &planes);
  // seeded starts (an addition; include/cspm.h "candidate fields"): hypotheses that win only where they cost less than what is there.
  // AddCandidates: one plane per pixel of a view (wid x hei, row-major; a plane with a non-finite value is no candidate);
  // AddCandidateDisparity: a CV_32FC1 / CV_64FC1 map offered as fronto-parallel planes, a non-finite or negative value being no
  // candidate.  Any number per view; kept here until the next PatchMatchSeeded / PatchMatchKeep, which merges them in this order.
  void AddCandidates(const RefView &view, const std::vector<Plane> &planes);
  void AddCandidateDisparity(const RefView &view, const Mat &disp);
  // the same map offered as SLANTED planes (an addition; include/cspm.h "plane fitting"): a weighted least-squares plane is fitted
  // around every value with this object's image of the view as guide (cspm_fit_planes_host; non-finite and negative values are no
  // nodes) and merged under the fit's `fitted` mask.  Throws for parameters the C ABI refuses.
  void AddCandidateDisparity(const RefView &view, const Mat &disp, const cspm_fit_params &params);
  // PatchMatchSeeded: InitRandomPlane, then the candidates merged, then iter_num iterations (cspm_pm_init, cspm_merge_planes_host,
  // cspm_patchmatch_warm).  PatchMatchKeep: the field already in the device context of plane_cost (LocalStereo, the previous frame's
  // run, SetPlanes) stays wherever InitRandomPlane's plane costs no less (cspm_pm_init_keep), then the candidates, then the iterations.
  // Begin / End as for PatchMatchFrom; one of this library's device costs only: a foreign IPlaneCost throws.
  void PatchMatchSeeded(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  void PatchMatchSeededBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  void PatchMatchKeep(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  void PatchMatchKeepBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp);
  // carried start for a moving rig (an addition; include/cspm.h "plane-field carry"): InitRandomPlane, then the final plane field of
  // `prev` -- the matcher of the previous frame, whose plane cost must still be alive -- carried across the motion X_this = R X_prev + t
  // between the two left cameras into this frame's disparity space and merged as candidates (cspm_pm_init, cspm_carry_planes with
  // merge = 1), then iter_num warm iterations (cspm_patchmatch_warm).  params == NULL: the defaults.  The two frames may differ in size.
  // Begin / End as for PatchMatchFrom; both plane costs must be this library's device costs on one GPU: anything else throws.
  void PatchMatchCarried(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp, const CSPatchMatch &prev, const cspm_calib &prev_calib,
                         const cspm_calib &calib, const double *R, const double *t, const cspm_carry_params *params = NULL);
  void PatchMatchCarriedBegin(const int &iter_num, const IPlaneCost *plane_cost, const bool &use_pp, const CSPatchMatch &prev, const cspm_calib &prev_calib,
                              const cspm_calib &calib, const double *R, const double *t, const cspm_carry_params *params = NULL);

  // additions (the reference seeds from time(NULL) and has one schedule)
  void set_seed(uint64_t seed) { seed_ = seed; }
  // schedule: CSPM_SCHED_*; rb_rounds: red-black / diffuse rounds per iteration; rb_neighbours: 2 or 4, under CSPM_SCHED_DIFFUSE 4, 8 or 20
  void set_schedule(int schedule, int rb_rounds = 1, int rb_neighbours = 4) {
    schedule_ = schedule;
    rb_rounds_ = rb_rounds;
    rb_neighbours_ = rb_neighbours;
  }
  // final plane field of a view, for callers that want sub-pixel disparities.  Both read the device context of the plane cost
  // the last PatchMatch ran on: call them while that object is alive (they throw otherwise).  They return the PLANE field --
  // PostProcessing (use_pp) works on the 8-bit maps only (cs_patchmatch.cc:508-588) and does not change it.
  void planes(const RefView &view, std::vector<Plane> *out, std::vector<double> *min_cost) const;
  // unquantised disparity a*x+b*y+c of every pixel, row-major (what PlaneToDisp rounds, cs_patchmatch.cc:590-601)
  void disparity(const RefView &view, std::vector<double> *out) const;
  // sub-pixel PostProcessing (an addition; include/cspm.h cspm_postprocess_f64): left-right check, fill and weighted median on the
  // unquantised disparities of both views, row-major; either output may be NULL.  Needs the cost object's images like use_pp (a
  // foreign IPlaneCost has them after a run with use_pp).  dis() and the plane field are not changed.
  void PostProcessedDisparity(std::vector<double> *l_out, std::vector<double> *r_out) const;
  // speckle filter of PostProcessing (an addition; include/cspm.h cspm_set_pp_speckle): between the left-right check and the fill,
  // connected components (4-neighbours whose disparities differ by at most max_diff) of at most max_size consistent pixels leave the
  // consistency mask, in use_pp's 8-bit maps and in PostProcessedDisparity alike.  max_size == 0 (the default) = no filter.  Kept
  // here and written into the cost object's context by every post-processing of this object.  Throws for max_size < 0 and for a
  // max_diff that is negative or not finite.
  void SetSpeckleFilter(int max_size, double max_diff);
  // median filter of PostProcessing (an addition; include/cspm.h cspm_set_pp_median): the call the reference keeps commented out at the
  // end of PostProcessing (cs_patchmatch.cc:573-575), as the last step after the weighted median, on every pixel of both views -- M8 on
  // use_pp's 8-bit maps, M64 on PostProcessedDisparity's.  r == 0 (the default) = no filter.  Kept here and written into the cost
  // object's context by every post-processing of this object.  Throws for r outside 0 .. CSPM_MEDIAN_MAX_RADIUS.
  void SetMedianFilter(int r);
  // edge-aware global smoothing of the sub-pixel PostProcessing (an addition; include/cspm.h cspm_set_pp_smooth): the last step of
  // PostProcessedDisparity and of the CSPM_GEOM_PP sources of Reproject and Synthesize, after the median filter, on both views.  use_pp's
  // 8-bit maps are not affected.  NULL or lambda == 0 (the default) = off.  Kept here and written into the cost object's context by
  // every post-processing of this object.  Throws for what cspm_set_pp_smooth refuses.
  void SetSmoothing(const cspm_smooth_params *params);
  // metric geometry of a view's final plane field (an addition; include/cspm.h "reprojection", cspm_reproject): source CSPM_GEOM_RAW (the
  // field's own disparities) or CSPM_GEOM_PP (the sub-pixel post-processed map, with this object's speckle and median settings); fit ==
  // NULL: the field's slopes, else slopes fitted to the map.  depth / keep: wid x hei row-major; xyz / normal: three planes of wid x hei;
  // cloud: the kept pixels' records in raster order.  Every output may be NULL.  Returns the number of kept pixels.  Reads the device
  // context of the plane cost the last run used, like disparity(); throws for what the C ABI refuses.
  size_t Reproject(const RefView &view, const cspm_calib &calib, const cspm_geom_params &params, int source, const cspm_fit_params *fit,
                   std::vector<double> *depth, std::vector<double> *xyz, std::vector<double> *normal, std::vector<uint8_t> *keep,
                   std::vector<cspm_point> *cloud) const;
  // a triangle mesh of a view's final plane field (an addition; include/cspm.h "triangle meshes", cspm_mesh): view, calib, params, source
  // and fit as for Reproject.  vertices: the mesh's cspm_point records in raster order; faces: their vertex numbers; quad: wid x hei quad
  // bytes.  Every output may be NULL.  Returns the number of faces; throws for what the C ABI refuses.
  size_t Mesh(const RefView &view, const cspm_calib &calib, const cspm_geom_params &params, const cspm_mesh_params &mesh_params, int source,
              const cspm_fit_params *fit, std::vector<cspm_point> *vertices, std::vector<cspm_face> *faces, std::vector<uint8_t> *quad) const;
  // view synthesis (cspm.h "view synthesis"): the scene from the camera at fraction t of the baseline (0 = the left
  // view, 1 = the right one), rendered from the stored plane field and the two images.  source as for Reproject.  bgr: a wid x hei 8UC3
  // image; disp: wid x hei row-major, NaN in holes; mask: wid x hei bytes, 0 hole, 1 / 2 one view, 3 both, 4 filled.  Every output may be
  // NULL.  Throws for what the C ABI refuses.
  void Synthesize(double t, const cspm_synth_params &params, int source, Mat *bgr, std::vector<double> *disp, std::vector<uint8_t> *mask) const;

 private:
  Mat img_[kViewNum], dis_[kViewNum];
  int wid_, hei_, max_dis_, dis_scale_;
  uint64_t seed_;
  int schedule_, rb_rounds_, rb_neighbours_;
  cspm_ctx *last_ctx_;
  cspm_ctx *own_ctx_;  // foreign IPlaneCost: the context that holds the plane field
  cspm_ctx *pending_ctx_;  // PatchMatchBegin without its PatchMatchEnd yet
  bool pending_pp_;
  int speckle_size_;
  double speckle_diff_;
  int median_r_;
  cspm_smooth_params smooth_;  // lambda == 0: off
  void ApplyPostFilters(cspm_ctx *ctx) const;
  std::vector<Plane> start_planes_[kViewNum];  // SetPlanes, not yet written into a context
  struct Candidates {  // AddCandidates / AddCandidateDisparity, not yet merged: 6 doubles per pixel and a mask (empty: every pixel)
    std::vector<double> norm_param;
    std::vector<uint8_t> mask;
  };
  std::vector<Candidates> candidates_[kViewNum];
  void WriteStartPlanes(cspm_ctx *ctx);
  void SeededBegin(bool keep, int iter_num, const IPlaneCost *plane_cost, bool use_pp);
  void PatchMatchForeign(int iter_num, const IPlaneCost *plane_cost, bool use_pp);
  CSPatchMatch(const CSPatchMatch &);
  CSPatchMatch(const std::pair<Mat, Mat> &rectified, const int &max_dis, const int &dis_scale);  // the raw-pair constructor delegates through here
};
