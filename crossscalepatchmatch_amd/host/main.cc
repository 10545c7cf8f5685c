// main.cc -- command line with the reference's ten flags and defaults (CSPM/main.cc:23-34) and its flow
// (main.cc:57-139): read the pair, construct the plane cost (timed), run PatchMatch, print "Total Time", write the
// two 8-bit maps.  Runs on the GPU through the host layer.  Extra flags: --seed --schedule --neighbours --device --iters --ca_name (local stereo)
// --warm_ca (local stereo, then --iters warm PatchMatch iterations) --l_seed_pfm --r_seed_pfm (disparity maps offered to the random start
// field as candidates) --seed_ca (local stereo, kept wherever the random start plane costs no less, then --iters iterations)
// --fit_radius --fit_max_diff --fit_merge (slanted planes fitted to the local-stereo field or to the seed maps before what follows)
// --seg_step --seg_compactness --seg_iters --seg_tau --seg_rounds --seg_warm_iters (one robust plane per superpixel of the field after the
// --iters iterations, merged where it costs less, then warm iterations; include/cspm.h "segment planes")
// --calib --l_ply --r_ply --l_depth_pfm --r_depth_pfm --geom_min_cos --geom_z_far --geom_left_frame --geom_fit_radius (metric depth maps and
// point clouds of the final plane field; include/cspm.h "reprojection") --l_mesh_ply --r_mesh_ply --mesh_max_diff --mesh_all_vertices
// (triangle meshes of the final plane field; include/cspm.h "triangle meshes") --synth_t --synth_png --synth_dis_pfm --synth_views --synth_max_stretch
// --synth_merge_diff --synth_fill (the scene rendered from a camera between the two views; include/cspm.h "view synthesis")
// --rig --rect_f --rect_w --rect_h --l_rect_file --r_rect_file (the inputs are RAW photographs of a calibrated rig, undistorted and
// row-aligned on the device before matching; include/cspm.h "rectification") --fuse_poses --fuse_ply --fuse_right --fuse_source
// --fuse_max_reproj --fuse_max_rel_depth --fuse_min_cos --fuse_min_views --fuse_no_suppress (with --batch_list and --calib or --rig: the
// depth maps of all pairs of the list fused into one point cloud in world coordinates; include/cspm.h "depth-map fusion") --fuse_register --fuse_register_window
// --fuse_poses_out --fuse_reg_iters --fuse_reg_stride --fuse_reg_max_dist --fuse_reg_huber (the poses of that fusion refined, or found
// without --fuse_poses, by registering the views against each other; include/cspm.h "depth-view registration") --carry_poses --carry_iters
// --carry_no_fill (with --batch_list and --calib or --rig: the list is one sequence of a moving rig, every pair starts from the previous
// pair's plane field carried across the motion; include/cspm.h "plane-field carry") --tsdf_ply --tsdf_origin --tsdf_dims --tsdf_voxel
// --tsdf_trunc --tsdf_max_weight --tsdf_min_cos --tsdf_register --tsdf_mesh_ply (with the fusion flags: the same views integrated in list
// order into one TSDF volume, its surface points written as PLY or as the vertices of a triangle mesh, and --fuse_register done frame to
// model; include/cspm.h "TSDF fusion" and "TSDF meshes").
#include "../../include/cspm.h"
#include "commfunc.h"
#include "cs_patchmatch.h"
#include "get_method.h"
#include "plane_cost/cspc.h"
#include "plane_cost/grd_pc.h"
#include "plane_cost/pre_cs_pc.h"
#include "plane_cost/pre_ss_pc.h"
#include "calib_io.h"
#include "depth_fusion.h"
#include "tsdf_volume.h"
#include "pfm_io.h"
#include "ply_io.h"
#include "rig_io.h"

#include <atomic>
#include <cmath>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>

// images
DEFINE_string(l_img_file, "l_img.png", "left input image (8-bit PNG / PPM / PGM)");
DEFINE_string(r_img_file, "r_img.png", "right input image");
DEFINE_string(l_dis_file, "l_dis.png", "left disparity map to write (8-bit)");
DEFINE_string(r_dis_file, "r_dis.png", "right disparity map to write (8-bit)");
// matching
DEFINE_int32(max_dis, 0, "disparity search range");
DEFINE_int32(dis_scale, 0, "factor applied to disparities before 8-bit quantisation");
DEFINE_string(cc_name, "CCName", "matching cost: GRD | CEN | CENGRD (census and GRD blended per cell; not in the reference)");
DEFINE_bool(cc_fused, false, "with --cc_name=CENGRD: compute the cells inside the PatchMatch kernels instead of materialising cost volumes "
                             "(same maps, no volume memory); no effect with any other --cc_name");
DEFINE_string(pc_name, "PRE", "plane cost family: PRE = PreSSPC / PreCSPC over --cc_name's cost volumes (the reference's main.cc); "
                              "IMG = GrdPC / CSPC, the volume-free colour + gradient costs (main.cc:106-107, commented out there)");
DEFINE_string(ca_name, "", "local stereo instead of PatchMatch: cost aggregation BOX | GF | BF over --cc_name's cost volumes, then "
              "cross-scale winner-take-all (empty: PatchMatch); not with --pc_name=IMG");
DEFINE_string(warm_ca, "", "warm-started PatchMatch: local stereo with cost aggregation BOX | GF | BF (as --ca_name), then --iters PatchMatch "
              "iterations from its plane field instead of the random init; needs --pc_name=PRE, not with --ca_name");
DEFINE_string(seed_ca, "", "seeded PatchMatch: local stereo with cost aggregation BOX | GF | BF (as --warm_ca), then the random start planes "
              "compete with its field pixel by pixel and the cheaper plane stays (keep-init), then --iters iterations; needs --pc_name=PRE, "
              "not with --warm_ca or --ca_name");
DEFINE_string(l_seed_pfm, "", "a float32 PFM disparity map of the left view offered to PatchMatch as candidates: after the random init (or the "
                              "keep-init of --seed_ca) a pixel takes the fronto-parallel plane of its value where that costs less; non-finite "
                              "or negative values are no candidates.  Not with --ca_name, --warm_ca or --batch_list");
DEFINE_string(r_seed_pfm, "", "the same for the right view (see --l_seed_pfm)");
DEFINE_int32(fit_radius, 0, "fit slanted planes (weighted least squares over a window of this half-width, 1 .. 17; include/cspm.h \"plane "
                           "fitting\") to the local-stereo field of --warm_ca / --seed_ca / --ca_name before what follows, and to the maps of "
                           "--l_seed_pfm / --r_seed_pfm instead of offering them as fronto-parallel planes; 0 = off.  An error without one of those");
DEFINE_double(fit_max_diff, 1.5, "with --fit_radius: a window pixel takes part in a fit when its disparity is within this of the centre's");
DEFINE_bool(fit_merge, false, "with --fit_radius and a local-stereo field: a fitted plane replaces the stored one only where it costs less "
                              "(default: every plane is replaced)");
DEFINE_int32(seg_step, 0, "segment planes (include/cspm.h \"segment planes\"): after the --iters PatchMatch iterations of any start, superpixels of "
                         "about this many pixels across (4 .. 64) each get one robustly fitted plane, offered to every pixel of the segment where "
                         "it costs less; --seg_warm_iters warm iterations follow, before post-processing and every output; 0 = off.  Not with "
                         "--ca_name; needs --pc_name=PRE or IMG");
DEFINE_int32(seg_compactness, 20, "with --seg_step: the weight of position against colour in the superpixel distance, 0 .. 255");
DEFINE_int32(seg_iters, 5, "with --seg_step: assignment + update rounds of the segmentation, 1 .. 16");
DEFINE_double(seg_tau, 1.0, "with --seg_step: the inlier threshold of the last re-fit, in disparities (it halves towards it round by round)");
DEFINE_int32(seg_rounds, 3, "with --seg_step: re-fits on the inliers, 0 .. 8 (0 = plain least squares)");
DEFINE_int32(seg_warm_iters, 1, "with --seg_step: warm PatchMatch iterations after the merge, 0 .. 15");
DEFINE_bool(use_cs, false, "cross-scale aggregation over a 5-level pyramid (PreCSPC) instead of PreSSPC");
DEFINE_bool(use_pp, false, "left-right check, hole filling and weighted median afterwards");
DEFINE_double(reg_lambda, 0.0, "cross-scale regularisation weight");
// not in the reference
DEFINE_int32(seed, 12345, "random seed (the reference uses the wall clock)");
DEFINE_string(schedule, "raster", "spatial propagation: raster (the reference's sweep) | redblack | diffuse (every pixel tries the planes of "
                                  "--neighbours near and far neighbours, read from a snapshot of the field; not in the reference)");
DEFINE_int32(neighbours, 8, "with --schedule=diffuse: candidates per pixel, 4 | 8 | 20 (include/cspm.h CSPM_SCHED_DIFFUSE); ignored by the other schedules");
DEFINE_int32(device, 0, "GPU index");
DEFINE_int32(iters, 3, "PatchMatch iterations (3 in the reference, main.cc:93)");
DEFINE_string(l_disp_pfm, "", "also write the left sub-pixel disparity map as float32 PFM: the unquantised plane disparity a*x+b*y+c, "
                              "BEFORE post-processing (--use_pp changes the 8-bit maps only, as in the reference)");
DEFINE_string(r_disp_pfm, "", "also write the right sub-pixel disparity map as float32 PFM (see --l_disp_pfm)");
DEFINE_bool(pp_pfm, false, "with --use_pp: the PFM maps (--l_disp_pfm / --r_disp_pfm, or the batch list's) receive the sub-pixel post-processed "
                           "disparities -- left-right check, fill and weighted median on a*x+b*y+c itself -- instead of the raw plane disparities");
DEFINE_int32(pp_speckle_size, 0, "with --use_pp: speckle filter between the left-right check and the fill -- connected components of at most "
                                 "this many consistent pixels are treated as inconsistent (filled and medianed); 0 = no filter.  Applies to the "
                                 "8-bit maps and, with --pp_pfm, to the PFM maps");
DEFINE_double(pp_speckle_diff, 1.0, "with --pp_speckle_size: two neighbouring pixels belong to one component when their disparities differ by at "
                                    "most this much (in disparity units, before --dis_scale)");
DEFINE_int32(pp_median, 0, "with --use_pp: radius of a median filter as the last post-processing step, on every pixel of both views (a "
                           "(2R+1) x (2R+1) window, border replicated); 0 = no filter, at most 7.  Applies to the 8-bit maps and, with "
                           "--pp_pfm, to the PFM maps");
DEFINE_double(pp_smooth_lambda, 0.0, "with --use_pp --pp_pfm: edge-aware global smoothing (the fast global smoother) as the last step of the sub-pixel "
                                     "post-processing, along the view's image, with confidence 1 where the pixel passed the left-right check; the "
                                     "smoothing strength, 0 = no smoothing.  Applies to the PFM maps only");
DEFINE_double(pp_smooth_sigma, 20.0, "with --pp_smooth_lambda: the colour scale of the guide weights exp(-(|dB|+|dG|+|dR|) / sigma)");
DEFINE_int32(pp_smooth_iters, 3, "with --pp_smooth_lambda: rounds of a horizontal and a vertical pass, 1 .. 8");
DEFINE_double(pp_smooth_fill_conf, 0.25, "with --pp_smooth_lambda: the confidence of a pixel that failed the left-right check, 0 .. 1");
DEFINE_string(calib, "", "a Middlebury-2014 calib.txt (cam0, cam1, doffs, baseline, width, height) of the pair: needed by the point-cloud and depth "
                         "outputs below.  When its width differs from the image width, f, cx, cy and doffs are scaled by image width / width");
DEFINE_string(l_ply, "", "write the left view's point cloud (binary little-endian PLY: x y z nx ny nz, red green blue; the baseline's unit) from the "
                         "final plane field: the raw plane disparities, or with --use_pp the sub-pixel post-processed map.  Needs --calib or --rig; "
                         "not with --batch_list");
DEFINE_string(rig, "", "a rig file (cam0, dist0, cam1, dist1, R, T, width, height; INTEGRATION.md \"rig files\"): --l_img_file / --r_img_file (or the "
                       "batch list's images) are then RAW photographs of that size, undistorted and row-aligned on the device before matching "
                       "(include/cspm.h \"rectification\"); the maps are built once per device context.  The calibration of the rectified pair is "
                       "derived from the rig and serves the point-cloud and depth outputs: not with --calib");
DEFINE_double(rect_f, 0.0, "with --rig: the focal length of the rectified pair in pixels; 0 = the mean of the four raw focal lengths");
DEFINE_int32(rect_w, 0, "with --rig: the width of the rectified pair; 0 = the raw width");
DEFINE_int32(rect_h, 0, "with --rig: the height of the rectified pair; 0 = the raw height");
DEFINE_string(l_rect_file, "", "with --rig: also write the rectified left image (8-bit colour PNG / PPM).  Not with --batch_list");
DEFINE_string(r_rect_file, "", "with --rig: also write the rectified right image");
DEFINE_string(r_ply, "", "the same for the right view, in its own camera frame unless --geom_left_frame");
DEFINE_string(l_depth_pfm, "", "write the left view's metric depth Z as float32 PFM, NaN where there is none (see --l_ply)");
DEFINE_string(r_depth_pfm, "", "the same for the right view");
DEFINE_string(l_mesh_ply, "", "write the left view's triangle mesh (binary little-endian PLY: the vertices of --l_ply, then the faces as vertex_indices "
                              "lists) from the final plane field (include/cspm.h \"triangle meshes\"): neighbouring pixels are connected where each one's "
                              "plane predicts the other's disparity.  Honours --use_pp and the --geom_* flags.  Needs --calib or --rig; not with --batch_list");
DEFINE_string(r_mesh_ply, "", "the same for the right view, in its own camera frame unless --geom_left_frame");
DEFINE_double(mesh_max_diff, 1.0, "meshes: connect two neighbouring pixels when each one's plane predicts the other's disparity to within this (>= 0)");
DEFINE_bool(mesh_all_vertices, false, "meshes: every point of the cloud is a vertex, not only the corners of the triangles");
DEFINE_double(geom_min_cos, 0.0, "point clouds: drop a pixel whose surface normal makes a smaller cosine than this with its view ray (0 .. 1; 0 = keep all)");
DEFINE_double(geom_z_far, 0.0, "point clouds and depth maps: no point beyond this depth (0 = no limit)");
DEFINE_bool(geom_left_frame, false, "the right view's points are given in the left camera's frame (X + baseline)");
DEFINE_int32(geom_fit_radius, 0, "normals from planes fitted to the disparity map over a window of this half-width (1 .. 17) instead of the plane "
                                "field's own slopes; 0 = the field's slopes");
DEFINE_double(synth_t, -1.0, "render the scene from the camera at this fraction of the baseline, 0 (the left view) .. 1 (the right view), from the "
                             "final plane field and the two images: the raw plane disparities, or with --use_pp the sub-pixel post-processed maps "
                             "(include/cspm.h \"view synthesis\").  Needs --synth_png or --synth_dis_pfm (with --batch_list: the list's columns); "
                             "negative = off");
DEFINE_string(synth_png, "", "with --synth_t: write the rendered view as an 8-bit colour PNG / PPM.  Not with --batch_list, whose lines name it");
DEFINE_string(synth_dis_pfm, "", "with --synth_t: write the rendered view's disparity map as float32 PFM, NaN in holes.  Not with --batch_list");
DEFINE_int32(synth_views, 3, "with --synth_t: the source views used, 1 = left, 2 = right, 3 = both");
DEFINE_double(synth_max_stretch, 4.0, "with --synth_t: a source pixel is dropped when its plane stretches it over more target pixels than this (>= 1)");
DEFINE_double(synth_merge_diff, 1.0, "with --synth_t: the two views are blended where their disparities differ by at most this (>= 0)");
DEFINE_bool(synth_fill, true, "with --synth_t: holes take the nearest pixel of their row on the background side");
DEFINE_string(fuse_poses, "", "with --batch_list and --calib (or --rig): fuse the depth maps of all pairs of the list into one point cloud "
                                "(include/cspm.h \"depth-map fusion\").  A poses file: line i holds the 12 numbers of the row-major camera -> world "
                                "[R | t] of pair i's RECTIFIED left camera (also with --rig); '#' starts a comment.  Needs --fuse_ply");
DEFINE_string(fuse_ply, "", "with --fuse_poses: the fused cloud in world coordinates, in the format of --l_ply");
DEFINE_bool(fuse_right, false, "with --fuse_poses: the right view of every pair is fused too");
DEFINE_string(fuse_source, "raw", "with --fuse_poses: raw = the plane field's own disparities, pp = the sub-pixel post-processed maps, consistent pixels only");
DEFINE_double(fuse_max_reproj, 2.0, "with --fuse_poses: the forward-backward reprojection error a confirming view may have, in pixels");
DEFINE_double(fuse_max_rel_depth, 0.01, "with --fuse_poses: the relative depth difference a confirming view may have");
DEFINE_double(fuse_min_cos, 0.0, "with --fuse_poses: the least cosine between the normals of a pixel and of a confirming view (0 = no test)");
DEFINE_int32(fuse_min_views, 2, "with --fuse_poses: a pixel is kept when at least this many other views confirm it");
DEFINE_bool(fuse_register, false, "with --batch_list, --fuse_ply and --calib or --rig: before the fusion the views are registered in list order on the device "
                                  "(include/cspm.h \"depth-view registration\"): view 0 keeps its pose (the identity without --fuse_poses), view i starts from "
                                  "the file's pose or, without --fuse_poses, from view i - 1's refined pose");
DEFINE_int32(fuse_register_window, 3, "with --fuse_register: a view is registered against this many left views before it");
DEFINE_string(fuse_poses_out, "", "with --fuse_register: the refined poses, in the format of --fuse_poses");
DEFINE_int32(fuse_reg_iters, 8, "with --fuse_register: Gauss-Newton iterations per view, 1 .. 64");
DEFINE_int32(fuse_reg_stride, 1, "with --fuse_register: every n-th pixel of a view in x and y is a sample");
DEFINE_double(fuse_reg_max_dist, 0.5, "with --fuse_register: the largest distance between a point and its associated point, in world units");
DEFINE_double(fuse_reg_huber, 0.05, "with --fuse_register: residuals beyond it are down-weighted, in world units (0 = plain least squares)");
DEFINE_string(carry_poses, "", "with --batch_list and --calib (or --rig): the list is ONE sequence of a moving rig, run in list order by one worker on "
                                "the first device.  A text file with one camera -> world pose of the left rectified camera per pair, in the format of "
                                "--fuse_poses (it may be the same file).  Pair 0 runs as without the flag; pair i runs the random init, then the plane field "
                                "of pair i - 1 carried across the motion and merged as candidates (include/cspm.h \"plane-field carry\"), then "
                                "--carry_iters warm iterations");
DEFINE_int32(carry_iters, 1, "with --carry_poses: warm PatchMatch iterations of every pair but the first, 0 .. 15");
DEFINE_bool(carry_no_fill, false, "with --carry_poses: a pixel no carried plane lands on gets no candidate instead of a neighbour's plane");
DEFINE_string(tsdf_ply, "", "with the fusion flags: the views the fusion collects are also integrated, in list order, into one TSDF volume "
                           "(include/cspm.h \"TSDF fusion\") and its surface points are written in the format of --fuse_ply.  Needs --tsdf_origin, "
                           "--tsdf_dims and --tsdf_voxel");
DEFINE_string(tsdf_mesh_ply, "", "with the fusion flags: the triangle mesh of the TSDF volume (include/cspm.h \"TSDF meshes\") in the format of --l_mesh_ply: "
                                "the vertices of --tsdf_ply, then the faces.  Needs what --tsdf_ply needs; --tsdf_ply itself may then be absent");
DEFINE_string(tsdf_origin, "", "with --tsdf_ply: x,y,z, the world corner of voxel (0, 0, 0)");
DEFINE_string(tsdf_dims, "", "with --tsdf_ply: nx,ny,nz, the number of voxels per axis");
DEFINE_double(tsdf_voxel, 0.0, "with --tsdf_ply: the edge length of a voxel, in world units");
DEFINE_double(tsdf_trunc, 0.0, "with --tsdf_ply: the truncation distance (0 = 4 voxels)");
DEFINE_double(tsdf_max_weight, 64.0, "with --tsdf_ply: a voxel's weight saturates here, 1 .. 16777216");
DEFINE_double(tsdf_min_cos, 0.0, "with --tsdf_ply: the least cosine between a pixel's normal and its view ray (0 = no test)");
DEFINE_bool(tsdf_register, false, "with --fuse_register and --tsdf_ply: view i is registered against a raycast of the volume built from views 0 .. i - 1, at "
                                  "view i - 1's pose (frame to model), instead of against the raw views before it");
DEFINE_bool(fuse_no_suppress, false, "with --fuse_poses: emit a surface from every view that sees it, not only from the first");
DEFINE_string(batch_list, "", "text file, one stereo pair per line: l_img r_img l_dis r_dis [l_pfm r_pfm [synth_png [synth_pfm]]] (the last two with "
                              "--synth_t, and then `-` skips an optional column); all pairs run with the "
                              "matching flags of this command line on one device context (buffers are reused between pairs). A pair "
                              "that fails is reported and the batch goes on; the exit code is non-zero if any pair failed");
DEFINE_int32(in_flight, 2, "with --batch_list: stereo pairs in flight per GPU (2 measured best on MI355X, 3 and 4 within 1.5 %).  Each is a worker thread with its own device context (one HIP stream): "
                           "it decodes its pair's PNGs, runs it and encodes the maps while the other workers' kernels keep the GPU busy (the raster "
                           "sweep of one pair leaves most CUs idle).  With 2 or more the sweep runs four-wavefront workgroups (CSPM_OPT_SWEEP_FOLD)");
DEFINE_string(devices, "", "with --batch_list: GPUs to spread the pairs over: a comma-separated list of indices (an index may repeat: that many "
                           "worker sets on that GPU) or `all`; empty = --device.  Pairs are independent: no data moves between GPUs");
DEFINE_bool(batch_skip_existing, false, "with --batch_list: skip the pairs whose output maps already exist (restart an interrupted batch)");
DEFINE_bool(quiet, false, "print errors and the batch summary only");

namespace {
const int kWindow = 35;  // main.cc:94
const int kScales = 5;   // main.cc:100

// --rig: what run() derived before any device was opened; read-only afterwards
bool g_rectify = false;
cspm_rig g_rig;
cspm_rectification g_rect;
cspm_calib g_rect_calib;
// --calib with --batch_list (the fusion): every pair of the list has this calibration
bool g_batch_calib = false;
CalibFile g_calib_file;
// --carry_poses: one pose per pair
std::vector<CameraPose> g_carry_poses;
std::unique_ptr<TsdfVolume> g_tsdf;  // --tsdf_ply: the volume the fusion's views are integrated into
// --fuse_poses: one pose per pair, and the views the workers collect (slot = pair index, or 2 * pair index + view with --fuse_right)
std::vector<CameraPose> g_poses;
std::unique_ptr<DepthFusion> g_fusion;

struct PairFiles {
  string l_img, r_img, l_dis, r_dis, l_pfm, r_pfm, synth_png, synth_pfm;
};

// One stereo pair on its way through the flow of main.cc:57-139, cut into the four stages a batch worker overlaps: load (decode the
// files), begin (construct the plane cost, enqueue PatchMatch on the calling thread's device slot), finish (wait, fetch the maps,
// release the cost object -- in batch mode its context is parked for the next pair), write (encode the maps).  `log` collects what the
// reference prints (a batch worker's lines are written out in one piece when its pair is done).
struct PairRun {
  PairFiles files;
  int line_no;
  size_t index;  // of the pair in the batch list
  Mat left, right;
  std::unique_ptr<IPlaneCost> cost;
  std::unique_ptr<CSPatchMatch> matcher;
  std::vector<double> pfm[kViewNum];
  std::vector<double> depth[kViewNum];      // --l_depth_pfm / --r_depth_pfm
  std::vector<cspm_point> cloud[kViewNum];  // --l_ply / --r_ply
  std::vector<cspm_point> mesh_v[kViewNum];  // --l_mesh_ply / --r_mesh_ply
  std::vector<cspm_face> mesh_f[kViewNum];
  Mat synth;                      // --synth_png
  std::vector<double> synth_dis;  // --synth_dis_pfm
  cspm_calib calib;
  double t0;
  int rc;
  std::ostringstream log;
  PairRun(const PairFiles &f, int line, size_t idx = 0) : files(f), line_no(line), index(idx), t0(0.0), rc(EXIT_SUCCESS) {}
};

void load(PairRun &p) {
  p.left = imread(p.files.l_img, CV_LOAD_IMAGE_COLOR);
  p.right = imread(p.files.r_img, CV_LOAD_IMAGE_COLOR);
  if (p.left.empty() || p.right.empty()) {
    // the reference waits for a key press here (main.cc:70-75); a batch tool must not
    p.log << "Error: can not open image\n";
    p.rc = EXIT_FAILURE;
  } else if (g_rectify && (p.left.cols != g_rig.raw_w || p.left.rows != g_rig.raw_h || p.right.cols != g_rig.raw_w || p.right.rows != g_rig.raw_h)) {
    p.log << "Error: the images are not of the rig's size " << g_rig.raw_w << " x " << g_rig.raw_h << "\n";
    p.rc = EXIT_FAILURE;
  }
}

// --ca_name / --warm_ca -> CSPM_CA_*, -1 for a name the library does not implement
int ca_method(const string &name) {
  if (name == "BOX") return CSPM_CA_BOX;
  if (name == "GF") return CSPM_CA_GF;
  if (name == "BF") return CSPM_CA_BF;
  return -1;
}

// prev: --carry_poses, the pair before this one in the sequence (its cost object still alive), or NULL
void begin(PairRun &p, CCMethod *cost_fn, const PairRun *prev = NULL) {
  if (p.rc != EXIT_SUCCESS) return;
  try {
    p.t0 = static_cast<double>(getTickCount());
    IPlaneCost *pc;
    if (FLAGS_pc_name == "IMG")
      pc = FLAGS_use_cs ? static_cast<IPlaneCost *>(new CSPC(p.left, p.right, FLAGS_max_dis, kWindow, kScales, FLAGS_reg_lambda))
                        : static_cast<IPlaneCost *>(new GrdPC(p.left, p.right, FLAGS_max_dis, kWindow));
    else
      pc = FLAGS_use_cs ? static_cast<IPlaneCost *>(new PreCSPC(p.left, p.right, FLAGS_max_dis, kWindow, kScales, cost_fn, FLAGS_reg_lambda))
                        : static_cast<IPlaneCost *>(new PreSSPC(p.left, p.right, FLAGS_max_dis, kWindow, cost_fn));
    p.cost.reset(pc);  // released on every path, exceptions included (batch mode goes on)
    if (g_rectify) {  // the slot's context has remapped the raw pair: everything from here on works on the rectified one
      const DevicePlaneCost *dev = dynamic_cast<const DevicePlaneCost *>(pc);
      if (!dev) throw std::runtime_error("--rig needs one of this library's plane costs");
      dev->LevelImages(&p.left, &p.right);
      p.calib = g_rect_calib;
    }
    p.matcher.reset(new CSPatchMatch(p.left, p.right, FLAGS_max_dis, FLAGS_dis_scale));
    p.matcher->set_seed(static_cast<uint64_t>(FLAGS_seed));
    p.matcher->SetSpeckleFilter(FLAGS_pp_speckle_size, FLAGS_pp_speckle_diff);
    p.matcher->SetMedianFilter(FLAGS_pp_median);
    const cspm_smooth_params smooth = {FLAGS_pp_smooth_lambda, FLAGS_pp_smooth_sigma, FLAGS_pp_smooth_iters, FLAGS_pp_smooth_fill_conf};
    p.matcher->SetSmoothing(&smooth);
    if (FLAGS_schedule == "diffuse") p.matcher->set_schedule(CSPM_SCHED_DIFFUSE, 1, FLAGS_neighbours);
    else p.matcher->set_schedule(FLAGS_schedule == "redblack" ? 1 : 0);
    cspm_fit_params fit;
    cspm_fit_default_params(&fit);
    fit.radius = FLAGS_fit_radius;
    fit.max_diff = FLAGS_fit_max_diff;
    const bool use_fit = FLAGS_fit_radius != 0;
    const string *seed_pfm[kViewNum] = {&FLAGS_l_seed_pfm, &FLAGS_r_seed_pfm};
    for (int v = 0; v < kViewNum; ++v) {
      if (seed_pfm[v]->empty()) continue;
      std::vector<double> d;
      int w = 0, h = 0;
      if (!ReadPFM(*seed_pfm[v], &d, &w, &h) || w != p.left.cols || h != p.left.rows)
        throw std::runtime_error("can not read " + *seed_pfm[v] + " as a single-channel PFM of the image size");
      Mat m(h, w, CV_64FC1);
      for (int y = 0; y < h; ++y) std::copy(d.begin() + (size_t)y * w, d.begin() + (size_t)(y + 1) * w, m.ptr<double>(y));
      if (use_fit) p.matcher->AddCandidateDisparity(v == 0 ? kLeft : kRight, m, fit);
      else p.matcher->AddCandidateDisparity(v == 0 ? kLeft : kRight, m);
    }
    if (prev) {  // init, the previous pair's field carried across the motion and merged, the warm iterations: all on the cost object's stream
      double R[9], t[3];
      const CameraPose &ps = g_carry_poses[prev->index], &pt = g_carry_poses[p.index];
      if (cspm_carry_relative_pose(ps.R, ps.t, pt.R, pt.t, R, t) != CSPM_OK) throw std::runtime_error(cspm_last_error(NULL));
      cspm_carry_params cp;
      cspm_carry_default_params(&cp);
      cp.fill = FLAGS_carry_no_fill ? 0 : 1;
      p.matcher->PatchMatchCarriedBegin(FLAGS_carry_iters, p.cost.get(), FLAGS_use_pp, *prev->matcher, prev->calib, p.calib, R, t, &cp);
    } else if (!FLAGS_seed_ca.empty()) {  // keep-init and the iterations are enqueued behind the local stereo on the cost object's stream
      p.matcher->LocalStereoBegin(ca_method(FLAGS_seed_ca), p.cost.get(), FLAGS_use_pp);
      if (use_fit) p.matcher->FitPlanes(p.cost.get(), fit, FLAGS_fit_merge);
      p.matcher->PatchMatchKeepBegin(FLAGS_iters, p.cost.get(), FLAGS_use_pp);
    } else if (!FLAGS_l_seed_pfm.empty() || !FLAGS_r_seed_pfm.empty()) {
      p.matcher->PatchMatchSeededBegin(FLAGS_iters, p.cost.get(), FLAGS_use_pp);
    } else if (!FLAGS_warm_ca.empty()) {  // the warm run is enqueued behind the local stereo on the cost object's stream
      p.matcher->LocalStereoBegin(ca_method(FLAGS_warm_ca), p.cost.get(), FLAGS_use_pp);
      if (use_fit) p.matcher->FitPlanes(p.cost.get(), fit, FLAGS_fit_merge);
      p.matcher->PatchMatchFromBegin(FLAGS_iters, p.cost.get(), FLAGS_use_pp);
    } else if (FLAGS_ca_name.empty()) {
      p.matcher->PatchMatchBegin(FLAGS_iters, p.cost.get(), FLAGS_use_pp);
    } else {
      p.matcher->LocalStereoBegin(ca_method(FLAGS_ca_name), p.cost.get(), FLAGS_use_pp);
      if (use_fit) p.matcher->FitPlanes(p.cost.get(), fit, FLAGS_fit_merge);
    }
    if (FLAGS_seg_step != 0) {  // enqueued behind the run on the cost object's stream; the merge leaves the field consistent
      cspm_seg_params seg;
      cspm_seg_default_params(&seg);
      seg.step = FLAGS_seg_step;
      seg.compactness = FLAGS_seg_compactness;
      seg.iters = FLAGS_seg_iters;
      seg.tau = FLAGS_seg_tau;
      seg.rounds = FLAGS_seg_rounds;
      p.matcher->SegmentPlanes(p.cost.get(), seg, true);
      if (FLAGS_seg_warm_iters > 0) p.matcher->PatchMatchFromBegin(FLAGS_seg_warm_iters, p.cost.get(), FLAGS_use_pp);
    }
  } catch (const std::exception &e) {  // a bad pair must not take the batch down
    p.log << "Error: " << e.what() << "\n";
    p.rc = EXIT_FAILURE;
    p.cost.reset();
  }
}

// keep_cost: the cost object (and with it the context that holds the plane field) outlives the call: the next pair of a sequence carries from it
void finish(PairRun &p, bool keep_cost = false) {
  if (p.rc == EXIT_SUCCESS) {
    try {
      p.matcher->PatchMatchEnd();
      const double seconds = (static_cast<double>(getTickCount()) - p.t0) / getTickFrequency();
      if (!FLAGS_quiet)
        p.log << "--------------------------------------------------------\n"
              << "Total Time: " << seconds << "\n"
              << "--------------------------------------------------------\n";
      const string *pfm[kViewNum] = {&p.files.l_pfm, &p.files.r_pfm};
      if (FLAGS_pp_pfm) {  // one call post-processes both views
        if (!pfm[0]->empty() || !pfm[1]->empty())
          p.matcher->PostProcessedDisparity(pfm[0]->empty() ? NULL : &p.pfm[0], pfm[1]->empty() ? NULL : &p.pfm[1]);
      } else {
        for (int v = 0; v < kViewNum; ++v)
          if (!pfm[v]->empty()) p.matcher->disparity(v == 0 ? kLeft : kRight, &p.pfm[v]);  // reads the cost object's context: before it goes
      }
      const string *ply[kViewNum] = {&FLAGS_l_ply, &FLAGS_r_ply}, *dpfm[kViewNum] = {&FLAGS_l_depth_pfm, &FLAGS_r_depth_pfm};
      const string *mply[kViewNum] = {&FLAGS_l_mesh_ply, &FLAGS_r_mesh_ply};
      for (int v = 0; v < kViewNum; ++v) {  // reads the cost object's context: before it goes
        if (ply[v]->empty() && dpfm[v]->empty() && mply[v]->empty()) continue;
        cspm_geom_params g;
        cspm_geom_default_params(&g);
        g.min_cos = FLAGS_geom_min_cos;
        if (FLAGS_geom_z_far > 0.0) g.z_far = FLAGS_geom_z_far;
        g.left_frame = FLAGS_geom_left_frame ? 1 : 0;
        cspm_fit_params fit;
        cspm_fit_default_params(&fit);
        fit.radius = FLAGS_geom_fit_radius;
        if (!mply[v]->empty()) {
          cspm_mesh_params mp;
          cspm_mesh_default_params(&mp);
          mp.max_diff = FLAGS_mesh_max_diff;
          mp.all_vertices = FLAGS_mesh_all_vertices ? 1 : 0;
          const double m0 = static_cast<double>(getTickCount());
          p.matcher->Mesh(v == 0 ? kLeft : kRight, p.calib, g, mp, FLAGS_use_pp ? CSPM_GEOM_PP : CSPM_GEOM_RAW, FLAGS_geom_fit_radius != 0 ? &fit : NULL,
                          &p.mesh_v[v], &p.mesh_f[v], NULL);
          if (!FLAGS_quiet)
            p.log << "Mesh, view " << v << ": " << p.mesh_v[v].size() << " vertices, " << p.mesh_f[v].size() << " faces, "
                  << (static_cast<double>(getTickCount()) - m0) / getTickFrequency() * 1e3 << " ms\n";
        }
        if (ply[v]->empty() && dpfm[v]->empty()) continue;
        const double g0 = static_cast<double>(getTickCount());
        const size_t count = p.matcher->Reproject(v == 0 ? kLeft : kRight, p.calib, g, FLAGS_use_pp ? CSPM_GEOM_PP : CSPM_GEOM_RAW,
                                                  FLAGS_geom_fit_radius != 0 ? &fit : NULL, dpfm[v]->empty() ? NULL : &p.depth[v], NULL, NULL, NULL,
                                                  ply[v]->empty() ? NULL : &p.cloud[v]);
        if (!FLAGS_quiet)
          p.log << "Reprojection, view " << v << ": " << count << " points, " << (static_cast<double>(getTickCount()) - g0) / getTickFrequency() * 1e3
                << " ms\n";
      }
      if (g_fusion) {  // reads the cost object's context: before it goes
        cspm_geom_params g;
        cspm_geom_default_params(&g);
        g.min_cos = FLAGS_geom_min_cos;
        if (FLAGS_geom_z_far > 0.0) g.z_far = FLAGS_geom_z_far;
        const bool pp = FLAGS_fuse_source == "pp";
        g.consistent_only = pp ? 1 : 0;
        cspm_fit_params fit;
        cspm_fit_default_params(&fit);
        fit.radius = FLAGS_geom_fit_radius;
        const int views = FLAGS_fuse_right ? 2 : 1;
        for (int v = 0; v < views; ++v) {
          std::vector<double> depth, normal;
          std::vector<uint8_t> keep;
          p.matcher->Reproject(v == 0 ? kLeft : kRight, p.calib, g, pp ? CSPM_GEOM_PP : CSPM_GEOM_RAW, FLAGS_geom_fit_radius != 0 ? &fit : NULL, &depth, NULL,
                               &normal, &keep, NULL);
          const Mat &img = v == 0 ? p.left : p.right;
          g_fusion->SetPairView(p.index * views + v, v, p.calib, g_poses[p.index], img.cols, img.rows, depth, keep, normal, img.ptr<unsigned char>(0), img.step);
        }
      }
      if (FLAGS_synth_t >= 0.0 && (!p.files.synth_png.empty() || !p.files.synth_pfm.empty())) {  // reads the cost object's context: before it goes
        cspm_synth_params sp;
        cspm_synth_default_params(&sp);
        sp.views = FLAGS_synth_views;
        sp.max_stretch = FLAGS_synth_max_stretch;
        sp.merge_diff = FLAGS_synth_merge_diff;
        sp.fill = FLAGS_synth_fill ? 1 : 0;
        const double s0 = static_cast<double>(getTickCount());
        p.matcher->Synthesize(FLAGS_synth_t, sp, FLAGS_use_pp ? CSPM_GEOM_PP : CSPM_GEOM_RAW, p.files.synth_png.empty() ? NULL : &p.synth,
                              p.files.synth_pfm.empty() ? NULL : &p.synth_dis, NULL);
        if (!FLAGS_quiet)
          p.log << "View synthesis, t = " << FLAGS_synth_t << ": " << (static_cast<double>(getTickCount()) - s0) / getTickFrequency() * 1e3 << " ms\n";
      }
    } catch (const std::exception &e) {
      p.log << "Error: " << e.what() << "\n";
      p.rc = EXIT_FAILURE;
    }
  }
  if (!keep_cost) p.cost.reset();
}

void write(PairRun &p) {
  if (p.rc != EXIT_SUCCESS) return;
  bool written = imwrite(p.files.l_dis, p.matcher->dis(kLeft)) && imwrite(p.files.r_dis, p.matcher->dis(kRight));
  const string *pfm[kViewNum] = {&p.files.l_pfm, &p.files.r_pfm};
  for (int v = 0; v < kViewNum && written; ++v)
    if (!pfm[v]->empty()) written = WritePFM(*pfm[v], p.pfm[v].data(), p.left.cols, p.left.rows);
  const string *ply[kViewNum] = {&FLAGS_l_ply, &FLAGS_r_ply}, *dpfm[kViewNum] = {&FLAGS_l_depth_pfm, &FLAGS_r_depth_pfm};
  for (int v = 0; v < kViewNum && written; ++v) {
    if (!dpfm[v]->empty()) written = WritePFM(*dpfm[v], p.depth[v].data(), p.left.cols, p.left.rows);
    if (written && !ply[v]->empty()) written = WritePLY(*ply[v], p.cloud[v].data(), p.cloud[v].size());
    const string &mply = v == 0 ? FLAGS_l_mesh_ply : FLAGS_r_mesh_ply;
    if (written && !mply.empty()) written = WritePLYMesh(mply, p.mesh_v[v].data(), p.mesh_v[v].size(), p.mesh_f[v].data(), p.mesh_f[v].size());
  }
  if (written && g_rectify && !FLAGS_l_rect_file.empty()) written = imwrite(FLAGS_l_rect_file, p.left);
  if (written && g_rectify && !FLAGS_r_rect_file.empty()) written = imwrite(FLAGS_r_rect_file, p.right);
  if (written && !p.synth.empty()) written = imwrite(p.files.synth_png, p.synth);
  if (written && !p.synth_dis.empty()) written = WritePFM(p.files.synth_pfm, p.synth_dis.data(), p.left.cols, p.left.rows);
  if (!written) {
    p.log << "Error: can not write disparity maps\n";
    p.rc = EXIT_FAILURE;
  }
}

struct BatchJob {
  PairFiles files;
  int line_no;
};

// --devices: "" -> {--device}; "all" -> every GPU; "0,1,1" -> those indices (repeats allowed).  Empty result = bad flag.
std::vector<int> parse_devices() {
  std::vector<int> out;
  const int n = DeviceSlot::device_count();
  if (FLAGS_devices.empty()) {
    if (FLAGS_device >= 0 && FLAGS_device < n) out.push_back(FLAGS_device);
    return out;
  }
  if (FLAGS_devices == "all") {
    for (int d = 0; d < n; ++d) out.push_back(d);
    return out;
  }
  std::istringstream is(FLAGS_devices);
  string tok;
  while (std::getline(is, tok, ',')) {
    char *end = NULL;
    const long d = std::strtol(tok.c_str(), &end, 10);
    if (tok.empty() || *end || d < 0 || d >= n) return std::vector<int>();
    out.push_back(static_cast<int>(d));
  }
  return out;
}

// The batch: pairs are independent units.  One worker thread per (entry of --devices, slot of --in_flight), each with
// its own DeviceSlot -- GPU index, parked context whose buffers the next pair of the worker takes over, whether it shares its GPU -- and
// its own CCMethod object; the workers pull pairs from one queue.  A worker blocks on its own pair only (cspm_ctx = one HIP stream), so
// file decoding / encoding and the serial phases of one pair overlap with the kernels of the others.  Results do not depend on the
// worker or GPU a pair lands on (same seed, same kernels): the maps equal the one-pair-at-a-time run bit for bit.
int run_batch(const std::vector<BatchJob> &jobs, int skipped, int bad_lines) {
  const std::vector<int> devices = parse_devices();
  if (devices.empty()) {
    cout << "Error: --devices must be `all` or a comma-separated list of GPU indices below " << DeviceSlot::device_count()
         << " (--device likewise); this node has " << DeviceSlot::device_count() << " usable GPU(s)\n";
    return EXIT_FAILURE;
  }
  const int per_gpu = std::max(1, FLAGS_in_flight);
  std::vector<int> on_gpu(DeviceSlot::device_count() > 0 ? DeviceSlot::device_count() : 1, 0);  // pairs in flight per physical GPU
  for (size_t i = 0; i < devices.size(); ++i) on_gpu[devices[i]] += per_gpu;
  std::atomic<size_t> next(0);
  std::atomic<int> failed(bad_lines), done(0);
  std::atomic<long long> sweep_fallbacks(0), volume_fallbacks(0);
  std::mutex out_mutex;
  const double t0 = static_cast<double>(getTickCount());
  auto worker = [&](int device) {
    DeviceSlot slot(device, /*keep_context=*/true, /*shared_gpu=*/on_gpu[device] >= 2);
    if (g_rectify) slot.SetRectification(&g_rig, &g_rect);  // one rig: the worker's parked context keeps its maps from pair to pair
    DeviceSlot::Use use(slot);
    const std::unique_ptr<CCMethod> cost_fn(GetCCType(FLAGS_cc_name));  // NULL for unknown names, rejected by the cost constructors
    if (CenGrdCC *cg = dynamic_cast<CenGrdCC *>(cost_fn.get())) cg->set_fused(FLAGS_cc_fused);
    // the next pair of the queue, decoded; a pair whose files cannot be read is reported at once and the worker moves on
    auto report = [&](PairRun &p) {
      if (p.rc != EXIT_SUCCESS) {
        ++failed;
        p.log << "Pair FAILED (line " << p.line_no << "): " << p.files.l_img << " " << p.files.r_img << "\n";
      }
      ++done;
      std::lock_guard<std::mutex> lock(out_mutex);
      cout << p.log.str() << std::flush;
    };
    auto next_loaded = [&]() -> std::unique_ptr<PairRun> {
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= jobs.size()) return std::unique_ptr<PairRun>();
        std::unique_ptr<PairRun> p(new PairRun(jobs[k].files, jobs[k].line_no, k));
        if (!FLAGS_quiet) p->log << "Load Image: " << p->files.l_img << " " << p->files.r_img << "\n";
        load(*p);
        if (g_batch_calib && p->rc == EXIT_SUCCESS) p->calib = ScaledCalib(g_calib_file, p->left.cols);
        if (p->rc == EXIT_SUCCESS) return p;
        report(*p);
      }
    };
    // software pipeline: while pair k is on the GPU the worker decodes pair k+1; as soon as k's maps are on the host, k+1 is
    // enqueued (on the context k just parked) and only then are k's maps encoded and written -- the worker's stream idles for the
    // download and the upload only, not for the files
    try {
      std::unique_ptr<PairRun> cur = next_loaded();
      if (cur) begin(*cur, cost_fn.get());
      while (cur) {
        std::unique_ptr<PairRun> nxt = next_loaded();
        finish(*cur);
        if (nxt) begin(*nxt, cost_fn.get());
        write(*cur);
        report(*cur);
        cur = std::move(nxt);
      }
    } catch (const std::exception &e) {  // the stages catch per pair; what still gets here (out of memory on the host ...) ends this worker, not the process
      ++failed;
      std::lock_guard<std::mutex> lock(out_mutex);
      cout << "Error: batch worker on GPU " << device << " stopped: " << e.what() << "\n" << std::flush;
    }
    slot.release();
    sweep_fallbacks += slot.sweep_fallbacks();
    volume_fallbacks += slot.volume_fallbacks();
  };
  std::vector<std::thread> threads;
  const size_t want = devices.size() * static_cast<size_t>(per_gpu);
  for (size_t t = 0; t < std::min(want, std::max<size_t>(jobs.size(), 1)); ++t) threads.emplace_back(worker, devices[t % devices.size()]);
  for (size_t t = 0; t < threads.size(); ++t) threads[t].join();
  const double seconds = (static_cast<double>(getTickCount()) - t0) / getTickFrequency();
  cout << "Batch: " << done.load() + bad_lines << " pairs in " << seconds << " s, " << failed.load() << " failed, " << skipped << " skipped\n";
  if (!FLAGS_quiet) {
    cout << "Batch workers: " << threads.size() << " (" << devices.size() << " GPU entr" << (devices.size() == 1 ? "y" : "ies") << " x " << per_gpu
         << " in flight), " << (done.load() ? seconds * 1e3 / done.load() : 0.0) << " ms per pair end to end, files included\n";
    cout << "Batch fallbacks: " << sweep_fallbacks.load() << " raster sweeps repeated after a hand-over timeout, " << volume_fallbacks.load()
         << " optional volumes given up\n";
  }
  if (g_fusion && failed.load() == 0) {  // all pairs are done: the views are fused in list order, whatever worker or GPU produced them
    try {
      const cspm_fuse_params fp = {FLAGS_fuse_max_reproj, FLAGS_fuse_max_rel_depth, FLAGS_fuse_min_cos, FLAGS_fuse_min_views, FLAGS_fuse_no_suppress ? 0 : 1};
      std::vector<cspm_point> cloud;
      if (FLAGS_fuse_register) {
        cspm_reg_params rp;
        cspm_reg_default_params(&rp);
        rp.iters = FLAGS_fuse_reg_iters; rp.stride = FLAGS_fuse_reg_stride; rp.max_dist = FLAGS_fuse_reg_max_dist; rp.huber = FLAGS_fuse_reg_huber;
        const int per_pair = FLAGS_fuse_right ? 2 : 1;
        const size_t pairs = g_fusion->size() / per_pair;
        std::vector<std::vector<cspm_reg_iter> > recs;
        const double r0 = static_cast<double>(getTickCount());
        if (FLAGS_tsdf_register) g_tsdf->Register(devices[0], g_fusion.get(), rp, per_pair, FLAGS_fuse_poses.empty(), &recs);
        else g_fusion->Register(devices[0], rp, FLAGS_fuse_register_window, per_pair, FLAGS_fuse_poses.empty(), &recs);
        if (!FLAGS_quiet) {
          for (size_t i = 1; i < pairs; ++i) {
            int taken = 0;
            for (size_t k = 0; k < recs[i].size(); ++k) taken += recs[i][k].status == 0;
            cout << "Registration, pair " << i << ": " << taken << " of " << recs[i].size() << " steps taken, " << recs[i].back().pairs << " pairs, cost "
                 << recs[i].back().cost << "\n";
          }
          cout << "Registration: " << pairs << " pairs, " << (static_cast<double>(getTickCount()) - r0) / getTickFrequency() * 1e3 << " ms\n";
        }
        if (!FLAGS_fuse_poses_out.empty()) {
          FILE *fp_out = fopen(FLAGS_fuse_poses_out.c_str(), "w");
          if (!fp_out) {
            cout << "Error: can not write " << FLAGS_fuse_poses_out << "\n";
            return EXIT_FAILURE;
          }
          for (size_t i = 0; i < pairs; ++i) {
            const CameraPose q = g_fusion->LeftPose(i, per_pair);
            for (int r = 0; r < 3; ++r)
              fprintf(fp_out, "%.17g %.17g %.17g %.17g%s", q.R[3 * r], q.R[3 * r + 1], q.R[3 * r + 2], q.t[r], r == 2 ? "\n" : "  ");
          }
          fclose(fp_out);
        }
      }
      const double f0 = static_cast<double>(getTickCount());
      const size_t count = g_fusion->Fuse(devices[0], fp, &cloud, NULL);
      if (!FLAGS_quiet)
        cout << "Fusion: " << g_fusion->size() << " views, " << count << " points, " << (static_cast<double>(getTickCount()) - f0) / getTickFrequency() * 1e3
             << " ms\n";
      if (!WritePLY(FLAGS_fuse_ply, cloud.data(), cloud.size())) {
        cout << "Error: can not write " << FLAGS_fuse_ply << "\n";
        return EXIT_FAILURE;
      }
      if (g_tsdf && !FLAGS_tsdf_ply.empty()) {  // the same views in the same list order, whatever worker or GPU produced them
        const double s0 = static_cast<double>(getTickCount());
        std::vector<cspm_point> surface;
        const size_t points = g_tsdf->Fuse(devices[0], *g_fusion, &surface);
        if (!FLAGS_quiet)
          cout << "TSDF: " << g_fusion->size() << " views, " << points << " surface points, " << (static_cast<double>(getTickCount()) - s0) / getTickFrequency() * 1e3
               << " ms\n";
        if (!WritePLY(FLAGS_tsdf_ply, surface.data(), surface.size())) {
          cout << "Error: can not write " << FLAGS_tsdf_ply << "\n";
          return EXIT_FAILURE;
        }
      }
      if (g_tsdf && !FLAGS_tsdf_mesh_ply.empty()) {
        const double s0 = static_cast<double>(getTickCount());
        std::vector<cspm_point> vertices;
        std::vector<cspm_face> faces;
        g_tsdf->Mesh(devices[0], *g_fusion, &vertices, &faces);
        if (!FLAGS_quiet)
          cout << "TSDF mesh: " << g_fusion->size() << " views, " << vertices.size() << " vertices, " << faces.size() << " faces, "
               << (static_cast<double>(getTickCount()) - s0) / getTickFrequency() * 1e3 << " ms\n";
        if (!WritePLYMesh(FLAGS_tsdf_mesh_ply, vertices.data(), vertices.size(), faces.data(), faces.size())) {
          cout << "Error: can not write " << FLAGS_tsdf_mesh_ply << "\n";
          return EXIT_FAILURE;
        }
      }
    } catch (const std::exception &e) {
      cout << "Error: " << e.what() << "\n";
      return EXIT_FAILURE;
    }
  } else if (g_fusion) {
    cout << "Error: no fusion: not every pair of the list succeeded\n";
  }
  return failed.load() ? EXIT_FAILURE : EXIT_SUCCESS;
}

// --carry_poses: the list is one sequence.  One worker on the first device, two device slots used alternately: pair i's context takes
// its start from pair i - 1's, which is released (parked for pair i + 1) as soon as the carry is enqueued behind it.
int run_sequence(const std::vector<BatchJob> &jobs) {
  const std::vector<int> devices = parse_devices();
  if (devices.empty()) {
    cout << "Error: --devices must be `all` or a comma-separated list of GPU indices below " << DeviceSlot::device_count()
         << " (--device likewise); this node has " << DeviceSlot::device_count() << " usable GPU(s)\n";
    return EXIT_FAILURE;
  }
  cout << "Sequence: --carry_poses runs the list in order on GPU " << devices[0] << " with two contexts; --in_flight does not apply\n";
  DeviceSlot slot_a(devices[0], /*keep_context=*/true), slot_b(devices[0], /*keep_context=*/true);
  DeviceSlot *const slots[2] = {&slot_a, &slot_b};
  const std::unique_ptr<CCMethod> cost_fn(GetCCType(FLAGS_cc_name));
  if (CenGrdCC *cg = dynamic_cast<CenGrdCC *>(cost_fn.get())) cg->set_fused(FLAGS_cc_fused);
  int failed = 0;
  const double t0 = static_cast<double>(getTickCount());
  std::unique_ptr<PairRun> prev;
  for (size_t k = 0; k < jobs.size(); ++k) {
    std::unique_ptr<PairRun> cur(new PairRun(jobs[k].files, jobs[k].line_no, k));
    if (!FLAGS_quiet) cur->log << "Load Image: " << cur->files.l_img << " " << cur->files.r_img << "\n";
    load(*cur);
    if (g_batch_calib && cur->rc == EXIT_SUCCESS) cur->calib = ScaledCalib(g_calib_file, cur->left.cols);
    {
      DeviceSlot &slot = *slots[k & 1];
      if (g_rectify) slot.SetRectification(&g_rig, &g_rect);
      DeviceSlot::Use use(slot);
      begin(*cur, cost_fn.get(), prev.get());
    }
    prev.reset();  // the carry is enqueued: the previous pair's context is parked for the pair after this one
    finish(*cur, /*keep_cost=*/true);
    write(*cur);
    if (cur->rc != EXIT_SUCCESS) {
      ++failed;
      cur->log << "Pair FAILED (line " << cur->line_no << "): " << cur->files.l_img << " " << cur->files.r_img << "\n";
    } else if (!FLAGS_quiet) {
      cur->log << (k == 0 ? "Sequence pair 0: cold start\n" : "Sequence pair: carried start\n");
    }
    cout << cur->log.str() << std::flush;
    if (cur->rc == EXIT_SUCCESS) prev = std::move(cur);  // a failed pair breaks the chain: the next one starts cold
  }
  prev.reset();
  slot_a.release();
  slot_b.release();
  const double seconds = (static_cast<double>(getTickCount()) - t0) / getTickFrequency();
  cout << "Batch: " << jobs.size() << " pairs in " << seconds << " s, " << failed << " failed, 0 skipped\n";
  return failed ? EXIT_FAILURE : EXIT_SUCCESS;
}

int run() {
  if (FLAGS_pp_pfm && !FLAGS_use_pp) {  // checked before anything opens a device
    cout << "Error: --pp_pfm post-processes the PFM maps and needs --use_pp\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_pp_speckle_size != 0 && !FLAGS_use_pp) {
    cout << "Error: --pp_speckle_size filters the post-processing's consistency masks and needs --use_pp\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_pp_speckle_size < 0 || !(FLAGS_pp_speckle_diff >= 0.0) || !std::isfinite(FLAGS_pp_speckle_diff)) {
    cout << "Error: --pp_speckle_size must be >= 0 and --pp_speckle_diff finite and >= 0\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_pp_median != 0 && !FLAGS_use_pp) {
    cout << "Error: --pp_median filters the post-processed maps and needs --use_pp\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_pp_median < 0 || FLAGS_pp_median > CSPM_MEDIAN_MAX_RADIUS) {
    cout << "Error: --pp_median must be 0 .. " << CSPM_MEDIAN_MAX_RADIUS << " (got " << FLAGS_pp_median << ")\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_pp_smooth_lambda != 0.0 && !(FLAGS_use_pp && FLAGS_pp_pfm)) {
    cout << "Error: --pp_smooth_lambda smooths the sub-pixel post-processed PFM maps and needs --use_pp --pp_pfm\n";
    return EXIT_FAILURE;
  }
  if (!(FLAGS_pp_smooth_lambda >= 0.0) || !std::isfinite(FLAGS_pp_smooth_lambda) || !(FLAGS_pp_smooth_sigma > 0.0) || !std::isfinite(FLAGS_pp_smooth_sigma) ||
      FLAGS_pp_smooth_iters < 1 || FLAGS_pp_smooth_iters > 8 || !(FLAGS_pp_smooth_fill_conf >= 0.0 && FLAGS_pp_smooth_fill_conf <= 1.0)) {
    cout << "Error: --pp_smooth_lambda must be finite and >= 0, --pp_smooth_sigma finite and > 0, --pp_smooth_iters 1 .. 8 and "
            "--pp_smooth_fill_conf 0 .. 1\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_ca_name.empty() && ca_method(FLAGS_ca_name) < 0) {  // checked before anything opens a device
    cout << "Error: --ca_name must be BOX, GF or BF (got " << FLAGS_ca_name << ")\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_warm_ca.empty() && ca_method(FLAGS_warm_ca) < 0) {
    cout << "Error: --warm_ca must be BOX, GF or BF (got " << FLAGS_warm_ca << ")\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_warm_ca.empty() && (FLAGS_pc_name != "PRE" || !FLAGS_ca_name.empty())) {
    cout << "Error: --warm_ca needs --pc_name=PRE (cost volumes to aggregate) and no --ca_name\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_seed_ca.empty() && ca_method(FLAGS_seed_ca) < 0) {
    cout << "Error: --seed_ca must be BOX, GF or BF (got " << FLAGS_seed_ca << ")\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_seed_ca.empty() && (!FLAGS_warm_ca.empty() || !FLAGS_ca_name.empty())) {
    cout << "Error: --seed_ca is a start of its own: not with --warm_ca or --ca_name\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_seed_ca.empty() && FLAGS_pc_name != "PRE") {
    cout << "Error: --seed_ca needs --pc_name=PRE (cost volumes to aggregate)\n";
    return EXIT_FAILURE;
  }
  const bool seed_pfm = !FLAGS_l_seed_pfm.empty() || !FLAGS_r_seed_pfm.empty();
  if (seed_pfm && (!FLAGS_warm_ca.empty() || !FLAGS_ca_name.empty())) {
    cout << "Error: --l_seed_pfm / --r_seed_pfm are merged after a random init: not with --warm_ca or --ca_name\n";
    return EXIT_FAILURE;
  }
  if (seed_pfm && !FLAGS_batch_list.empty()) {
    cout << "Error: --l_seed_pfm / --r_seed_pfm belong to one pair: not with --batch_list\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_fit_radius != 0 && (FLAGS_fit_radius < 1 || FLAGS_fit_radius > 17 || !(FLAGS_fit_max_diff >= 0.0))) {
    cout << "Error: --fit_radius must be 1 .. 17 (0 = off) and --fit_max_diff >= 0\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_fit_radius != 0 && !seed_pfm && FLAGS_warm_ca.empty() && FLAGS_seed_ca.empty() && FLAGS_ca_name.empty()) {
    cout << "Error: --fit_radius fits planes to a local-stereo field or to seed maps: it needs --warm_ca, --seed_ca, --ca_name, --l_seed_pfm or "
            "--r_seed_pfm\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_fit_merge && FLAGS_fit_radius == 0) {
    cout << "Error: --fit_merge needs --fit_radius\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_seg_step != 0) {
    if (FLAGS_seg_step < 4 || FLAGS_seg_step > 64 || FLAGS_seg_compactness < 0 || FLAGS_seg_compactness > 255 || FLAGS_seg_iters < 1 || FLAGS_seg_iters > 16 ||
        !(FLAGS_seg_tau >= 0.0) || FLAGS_seg_rounds < 0 || FLAGS_seg_rounds > 8 || FLAGS_seg_warm_iters < 0 || FLAGS_seg_warm_iters > 15) {
      cout << "Error: --seg_step must be 4 .. 64 (0 = off), --seg_compactness 0 .. 255, --seg_iters 1 .. 16, --seg_tau >= 0, --seg_rounds 0 .. 8 and "
              "--seg_warm_iters 0 .. 15\n";
      return EXIT_FAILURE;
    }
    if (!FLAGS_ca_name.empty()) {
      cout << "Error: --seg_step merges segment planes into a PatchMatch field under its plane cost: not with --ca_name (use --warm_ca or --seed_ca)\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
      cout << "Error: --seg_step needs one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
      return EXIT_FAILURE;
    }
  }
  if ((seed_pfm || !FLAGS_seed_ca.empty()) && FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
    cout << "Error: seeded starts need one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_ca_name.empty() && FLAGS_pc_name == "IMG") {
    cout << "Error: --ca_name aggregates cost volumes; --pc_name=IMG (GrdPC / CSPC) has none\n";
    return EXIT_FAILURE;
  }
  const bool mesh_out = !FLAGS_l_mesh_ply.empty() || !FLAGS_r_mesh_ply.empty();
  const bool geom_out = !FLAGS_l_ply.empty() || !FLAGS_r_ply.empty() || !FLAGS_l_depth_pfm.empty() || !FLAGS_r_depth_pfm.empty() || mesh_out;
  if (!FLAGS_rig.empty() && !FLAGS_calib.empty()) {  // checked before anything opens a device
    cout << "Error: --rig derives the calibration of the rectified pair itself: not with --calib\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_rig.empty() && (FLAGS_rect_f != 0.0 || FLAGS_rect_w != 0 || FLAGS_rect_h != 0 || !FLAGS_l_rect_file.empty() || !FLAGS_r_rect_file.empty())) {
    cout << "Error: --rect_f / --rect_w / --rect_h / --l_rect_file / --r_rect_file need --rig\n";
    return EXIT_FAILURE;
  }
  if (!(FLAGS_rect_f >= 0.0) || !std::isfinite(FLAGS_rect_f) || FLAGS_rect_w < 0 || FLAGS_rect_h < 0) {
    cout << "Error: --rect_f must be finite and >= 0, --rect_w and --rect_h >= 0 (0 = automatic)\n";
    return EXIT_FAILURE;
  }
  if ((!FLAGS_l_rect_file.empty() || !FLAGS_r_rect_file.empty()) && !FLAGS_batch_list.empty()) {
    cout << "Error: --l_rect_file / --r_rect_file belong to one pair: not with --batch_list\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_rig.empty() && FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
    cout << "Error: --rig needs one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
    return EXIT_FAILURE;
  }
  if (geom_out && FLAGS_calib.empty() && FLAGS_rig.empty()) {
    cout << "Error: --l_ply / --r_ply / --l_depth_pfm / --r_depth_pfm / --l_mesh_ply / --r_mesh_ply need --calib or --rig\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_fuse_register && !FLAGS_fuse_poses_out.empty()) {
    cout << "Error: --fuse_poses_out writes the poses of --fuse_register\n";
    return EXIT_FAILURE;
  }
  const bool fusion = !FLAGS_fuse_poses.empty() || !FLAGS_fuse_ply.empty() || FLAGS_fuse_register;
  {  // the TSDF flags, checked before anything opens a device
    const bool tsdf_any = !FLAGS_tsdf_ply.empty() || !FLAGS_tsdf_mesh_ply.empty() || !FLAGS_tsdf_origin.empty() || !FLAGS_tsdf_dims.empty() || FLAGS_tsdf_voxel != 0.0 || FLAGS_tsdf_trunc != 0.0 ||
                          FLAGS_tsdf_max_weight != 64.0 || FLAGS_tsdf_min_cos != 0.0 || FLAGS_tsdf_register;
    if (tsdf_any && ((FLAGS_tsdf_ply.empty() && FLAGS_tsdf_mesh_ply.empty()) || FLAGS_tsdf_origin.empty() || FLAGS_tsdf_dims.empty() || !fusion)) {
      cout << "Error: the TSDF flags need --tsdf_ply, --tsdf_origin, --tsdf_dims, --tsdf_voxel and the fusion (--fuse_poses or --fuse_register, --fuse_ply); "
              "--tsdf_mesh_ply may stand for --tsdf_ply\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_tsdf_register && !FLAGS_fuse_register) {
      cout << "Error: --tsdf_register changes what --fuse_register registers against: it needs --fuse_register\n";
      return EXIT_FAILURE;
    }
    if (tsdf_any) {
      cspm_tsdf_params tp;
      cspm_tsdf_default_params(&tp);
      int dims[3];
      if (!ParseTsdfTriple(FLAGS_tsdf_origin.c_str(), tp.origin) || !ParseTsdfDims(FLAGS_tsdf_dims.c_str(), dims)) {
        cout << "Error: --tsdf_origin must be x,y,z and --tsdf_dims nx,ny,nz\n";
        return EXIT_FAILURE;
      }
      tp.nx = dims[0]; tp.ny = dims[1]; tp.nz = dims[2];
      tp.voxel = FLAGS_tsdf_voxel; tp.trunc = FLAGS_tsdf_trunc; tp.max_weight = FLAGS_tsdf_max_weight; tp.min_cos = FLAGS_tsdf_min_cos;
      const bool finite = std::isfinite(tp.origin[0]) && std::isfinite(tp.origin[1]) && std::isfinite(tp.origin[2]) && std::isfinite(tp.voxel) && std::isfinite(tp.trunc);
      if (!finite || !(tp.voxel > 0.0) || tp.nx < 1 || tp.ny < 1 || tp.nz < 1 || (long long)tp.nx * tp.ny >= (1LL << 31) ||
          (long long)tp.nx * tp.ny * tp.nz >= (1LL << 31) || !(tp.trunc >= 0.0) || !(tp.max_weight >= 1.0 && tp.max_weight <= 16777216.0) ||
          !(tp.min_cos >= 0.0 && tp.min_cos <= 1.0)) {
        cout << "Error: --tsdf_origin must be finite, --tsdf_voxel > 0, --tsdf_dims at least 1,1,1 with fewer than 2^31 voxels, --tsdf_trunc >= 0 (0 = 4 voxels), "
                "--tsdf_max_weight 1 .. 16777216 and --tsdf_min_cos 0 .. 1\n";
        return EXIT_FAILURE;
      }
      g_tsdf.reset(new TsdfVolume(tp));
    }
  }
  const bool carry = !FLAGS_carry_poses.empty();
  if (!carry && (FLAGS_carry_iters != 1 || FLAGS_carry_no_fill)) {  // checked before anything opens a device
    cout << "Error: --carry_iters and --carry_no_fill need --carry_poses\n";
    return EXIT_FAILURE;
  }
  if (carry) {
    if (FLAGS_batch_list.empty() || (FLAGS_calib.empty() && FLAGS_rig.empty())) {
      cout << "Error: --carry_poses needs --batch_list and --calib or --rig\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_carry_iters < 0 || FLAGS_carry_iters > 15) {
      cout << "Error: --carry_iters must be 0 .. 15\n";
      return EXIT_FAILURE;
    }
    if (fusion || FLAGS_batch_skip_existing || !FLAGS_ca_name.empty() || !FLAGS_warm_ca.empty() || !FLAGS_seed_ca.empty() || FLAGS_seg_step != 0) {
      cout << "Error: --carry_poses runs plain PatchMatch over every pair of the list: not with the fusion, --batch_skip_existing, --ca_name, --warm_ca, "
              "--seed_ca or --seg_step\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
      cout << "Error: --carry_poses needs one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
      return EXIT_FAILURE;
    }
    int bad_line = 0;
    if (!ReadPoseFile(FLAGS_carry_poses, &g_carry_poses, &bad_line)) {
      cout << "Error: can not read " << FLAGS_carry_poses << " as a poses file (12 numbers per line, the row-major [R | t])";
      if (bad_line) cout << ": line " << bad_line;
      cout << "\n";
      return EXIT_FAILURE;
    }
  }
  if ((geom_out || (!FLAGS_calib.empty() && !fusion && !carry)) && !FLAGS_batch_list.empty()) {
    cout << "Error: --calib and the point-cloud, depth and mesh outputs belong to one pair: not with --batch_list\n";
    return EXIT_FAILURE;
  }
  if (fusion) {  // checked before anything opens a device
    if (FLAGS_fuse_register) {
      if (FLAGS_fuse_ply.empty() || FLAGS_batch_list.empty() || (FLAGS_calib.empty() && FLAGS_rig.empty())) {
        cout << "Error: --fuse_register needs --fuse_ply, --batch_list and --calib or --rig\n";
        return EXIT_FAILURE;
      }
      if (FLAGS_fuse_reg_iters < 1 || FLAGS_fuse_reg_iters > CSPM_REG_MAX_ITERS || FLAGS_fuse_reg_stride < 1 || !(FLAGS_fuse_reg_max_dist >= 0.0) ||
          !(FLAGS_fuse_reg_huber >= 0.0) || FLAGS_fuse_register_window < 1 || FLAGS_fuse_register_window > CSPM_FUSE_MAX_VIEWS - 1) {
        cout << "Error: --fuse_reg_iters must be 1 .. " << CSPM_REG_MAX_ITERS << ", --fuse_reg_stride >= 1, --fuse_reg_max_dist and --fuse_reg_huber >= 0 and "
             << "--fuse_register_window 1 .. " << CSPM_FUSE_MAX_VIEWS - 1 << "\n";
        return EXIT_FAILURE;
      }
    } else if (FLAGS_fuse_poses.empty() || FLAGS_fuse_ply.empty() || FLAGS_batch_list.empty() || (FLAGS_calib.empty() && FLAGS_rig.empty())) {
      cout << "Error: the fusion needs --fuse_poses, --fuse_ply, --batch_list and --calib or --rig\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_fuse_source != "raw" && FLAGS_fuse_source != "pp") {
      cout << "Error: --fuse_source must be raw or pp\n";
      return EXIT_FAILURE;
    }
    if (!(FLAGS_fuse_max_reproj >= 0.0) || !(FLAGS_fuse_max_rel_depth >= 0.0) || !(FLAGS_fuse_min_cos >= 0.0 && FLAGS_fuse_min_cos <= 1.0) ||
        FLAGS_fuse_min_views < 0 || FLAGS_fuse_min_views > 63) {
      cout << "Error: --fuse_max_reproj and --fuse_max_rel_depth must be >= 0, --fuse_min_cos 0 .. 1 and --fuse_min_views 0 .. 63\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
      cout << "Error: the fusion needs one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_batch_skip_existing) {
      cout << "Error: the fusion needs every pair of the list: not with --batch_skip_existing\n";
      return EXIT_FAILURE;
    }
    int bad_line = 0;
    if (!FLAGS_fuse_poses.empty() && !ReadPoseFile(FLAGS_fuse_poses, &g_poses, &bad_line)) {
      cout << "Error: can not read " << FLAGS_fuse_poses << " as a poses file (12 numbers per line, the row-major [R | t])";
      if (bad_line) cout << ": line " << bad_line;
      cout << "\n";
      return EXIT_FAILURE;
    }
  }
  if (!(FLAGS_geom_min_cos >= 0.0 && FLAGS_geom_min_cos <= 1.0) || !(FLAGS_geom_z_far >= 0.0) || FLAGS_geom_fit_radius < 0 || FLAGS_geom_fit_radius > 17) {
    cout << "Error: --geom_min_cos must be 0 .. 1, --geom_z_far >= 0 (0 = no limit) and --geom_fit_radius 0 .. 17\n";
    return EXIT_FAILURE;
  }
  if (!(FLAGS_mesh_max_diff >= 0.0)) {
    cout << "Error: --mesh_max_diff must be >= 0\n";
    return EXIT_FAILURE;
  }
  if (geom_out && FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
    cout << "Error: the point-cloud and depth outputs need one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
    return EXIT_FAILURE;
  }
  const bool synth_flags = !FLAGS_synth_png.empty() || !FLAGS_synth_dis_pfm.empty();
  if (FLAGS_synth_t < 0.0 && synth_flags) {  // checked before anything opens a device
    cout << "Error: --synth_png / --synth_dis_pfm need --synth_t\n";
    return EXIT_FAILURE;
  }
  if (FLAGS_synth_t >= 0.0 || std::isnan(FLAGS_synth_t)) {
    if (!(FLAGS_synth_t <= 1.0) || FLAGS_synth_views < 1 || FLAGS_synth_views > 3 || !(FLAGS_synth_max_stretch >= 1.0) || !(FLAGS_synth_merge_diff >= 0.0)) {
      cout << "Error: --synth_t must be 0 .. 1, --synth_views 1 .. 3, --synth_max_stretch >= 1 and --synth_merge_diff >= 0\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_batch_list.empty() ? !synth_flags : synth_flags) {
      cout << "Error: --synth_t writes to --synth_png / --synth_dis_pfm for one pair, and to the list's columns 7 and 8 with --batch_list\n";
      return EXIT_FAILURE;
    }
    if (FLAGS_pc_name != "PRE" && FLAGS_pc_name != "IMG") {
      cout << "Error: view synthesis needs one of this library's plane costs (--pc_name=PRE or IMG), not " << FLAGS_pc_name << "\n";
      return EXIT_FAILURE;
    }
  }
  CalibFile &calib_file = g_calib_file;
  if (!FLAGS_calib.empty() && !ReadCalibFile(FLAGS_calib, &calib_file)) {
    cout << "Error: can not read " << FLAGS_calib << " as a Middlebury calib.txt (cam0, cam1, doffs, baseline, width, height)\n";
    return EXIT_FAILURE;
  }
  if (!FLAGS_rig.empty()) {  // the file and the derivation are host work: a bad rig is reported before a device is opened
    if (!ReadRigFile(FLAGS_rig, &g_rig)) {
      cout << "Error: can not read " << FLAGS_rig << " as a rig file (cam0, dist0, cam1, dist1, R, T, width, height)\n";
      return EXIT_FAILURE;
    }
    cspm_rect_params rp;
    cspm_rect_default_params(&rp);
    rp.f = FLAGS_rect_f;
    rp.w = FLAGS_rect_w;
    rp.h = FLAGS_rect_h;
    if (cspm_rectify_compute(&g_rig, &rp, &g_rect, &g_rect_calib) != CSPM_OK) {
      cout << "Error: " << FLAGS_rig << ": " << cspm_last_error(NULL) << "\n";
      return EXIT_FAILURE;
    }
    g_rectify = true;
    if (!FLAGS_quiet)
      cout << "Rectification: " << g_rig.raw_w << " x " << g_rig.raw_h << " raw -> " << g_rect.w << " x " << g_rect.h << ", f " << g_rect.f << ", cx "
           << g_rect.cx << ", cy " << g_rect.cy << ", baseline " << g_rect.baseline << "\n";
  }
  DevicePlaneCost::device = FLAGS_device;
  if (FLAGS_use_pp && !FLAGS_pp_pfm && !(FLAGS_l_disp_pfm.empty() && FLAGS_r_disp_pfm.empty()) && !FLAGS_quiet)
    cout << "Note: the PFM maps hold the plane disparities before post-processing (--pp_pfm writes the post-processed ones)\n";
  if (FLAGS_batch_list.empty()) {
    const std::unique_ptr<CCMethod> cost_fn(GetCCType(FLAGS_cc_name));  // NULL for unknown names, rejected by the cost constructors
    if (CenGrdCC *cg = dynamic_cast<CenGrdCC *>(cost_fn.get())) cg->set_fused(FLAGS_cc_fused);
    if (!FLAGS_quiet) cout << "Load Image: " << FLAGS_l_img_file << " " << FLAGS_r_img_file << "\n";
    PairRun p(PairFiles{FLAGS_l_img_file, FLAGS_r_img_file, FLAGS_l_dis_file, FLAGS_r_dis_file, FLAGS_l_disp_pfm, FLAGS_r_disp_pfm, FLAGS_synth_png,
                        FLAGS_synth_dis_pfm},
              0);
    load(p);
    if (!FLAGS_calib.empty() && p.rc == EXIT_SUCCESS) p.calib = ScaledCalib(calib_file, p.left.cols);
    if (g_rectify) DeviceSlot::current().SetRectification(&g_rig, &g_rect);
    begin(p, cost_fn.get());
    finish(p);
    write(p);
    cout << p.log.str();
    return p.rc;
  }
  std::ifstream list(FLAGS_batch_list.c_str());
  if (!list) {
    cout << "Error: can not open batch list " << FLAGS_batch_list << "\n";
    return EXIT_FAILURE;
  }
  std::vector<BatchJob> jobs;
  string line;
  int bad_lines = 0, skipped = 0, line_no = 0;
  while (std::getline(list, line)) {
    ++line_no;
    std::istringstream is(line);
    PairFiles f;
    if (!(is >> f.l_img)) continue;  // blank line
    if (f.l_img[0] == '#') continue;
    if (!(is >> f.r_img >> f.l_dis >> f.r_dis)) {
      cout << "Error: batch list line " << line_no << " needs l_img r_img l_dis r_dis: " << line << "\n";
      ++bad_lines;
      continue;
    }
    is >> f.l_pfm >> f.r_pfm >> f.synth_png >> f.synth_pfm;
    if (FLAGS_synth_t >= 0.0) {  // a list that names view-synthesis outputs may skip an earlier optional column with "-"
      string *opt[4] = {&f.l_pfm, &f.r_pfm, &f.synth_png, &f.synth_pfm};
      for (int k = 0; k < 4; ++k)
        if (*opt[k] == "-") opt[k]->clear();
    } else {
      f.synth_png.clear();
      f.synth_pfm.clear();
    }
    if (FLAGS_batch_skip_existing && std::ifstream(f.l_dis.c_str()).good() && std::ifstream(f.r_dis.c_str()).good()) {
      ++skipped;
      continue;
    }
    jobs.push_back(BatchJob{f, line_no});
  }
  if (fusion) {  // before any pair runs
    const size_t views = jobs.size() * (FLAGS_fuse_right ? 2 : 1);
    if (FLAGS_fuse_poses.empty()) {  // --fuse_register alone: every pair starts as the identity
      const CameraPose eye = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
      g_poses.assign(jobs.size(), eye);
    }
    if (bad_lines != 0 || g_poses.size() != jobs.size()) {
      cout << "Error: " << FLAGS_fuse_poses << " holds " << g_poses.size() << " poses, the batch list " << jobs.size() << " pairs"
           << (bad_lines ? " and lines that are no pairs" : "") << "\n";
      return EXIT_FAILURE;
    }
    if (views < 1 || views > CSPM_FUSE_MAX_VIEWS) {
      cout << "Error: the fusion takes 1 .. " << CSPM_FUSE_MAX_VIEWS << " views, the list asks for " << views << "\n";
      return EXIT_FAILURE;
    }
    g_batch_calib = !FLAGS_calib.empty();
    g_fusion.reset(new DepthFusion(views));
  }
  if (carry) {  // before any pair runs
    if (bad_lines != 0 || g_carry_poses.size() != jobs.size()) {
      cout << "Error: " << FLAGS_carry_poses << " holds " << g_carry_poses.size() << " poses, the batch list " << jobs.size() << " pairs"
           << (bad_lines ? " and lines that are no pairs" : "") << "\n";
      return EXIT_FAILURE;
    }
    g_batch_calib = !FLAGS_calib.empty();
    return run_sequence(jobs);
  }
  return run_batch(jobs, skipped, bad_lines);
}
}  // namespace

int main(int argc, char **argv) {
  // HIP maps streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues; two pair streams that share a queue run one after the other
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  gflags::ParseCommandLineFlags(&argc, &argv, true);
  if (!FLAGS_quiet) cout << "PatchMatch Stereo Matching (MI355X)" << endl;
  try {
    return run();
  } catch (const std::exception &e) {
    cout << "Error: " << e.what() << endl;
    return EXIT_FAILURE;
  }
}
