// cengrd_cc.h -- CenGrdCC: the combined census + gradient matching cost CENGRD, a third CCMethod behind the plugin slot.  The
// reference reserves such a slot (GetCCType("CG") / "BSM", CSPM/main.cc:47-54) and defines nothing behind it; the cell is this
// library's own definition (include/cspm.h):
//     cell = fma(CSPM_CENGRD_KAPPA, min(H, CSPM_CENGRD_TAU), G)     G = the device's GRD cell, H = CenCC's Hamming cell
// buildCV / buildRightCV keep the host-buffer contract and run the kernel of libcspm_hip.so (cspm_cengrd_build_cv_host);
// PreSSPC / PreCSPC recognise a CenGrdCC and build its cost on the device (cspm_build_cost_cengrd): with volumes, or -- fused() -- with
// the cells computed inside the PatchMatch kernels (CSPM_OPT_CENGRD_FUSED: identical planes and costs, no volume memory).
#pragma once
#include "../cc_method.h"

class CenGrdCC : public CCMethod {
 public:
  // device < 0 (default): the GPU of the calling thread's DeviceSlot at the time of the call (plane_cost/device_plane_cost.h)
  explicit CenGrdCC(int device = -1, bool fused = false) : device_(device), fused_(fused) {}
  ~CenGrdCC() {}
  bool fused() const { return fused_; }
  void set_fused(bool fused) { fused_ = fused; }
  void buildCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol);
  void buildRightCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *rCostVol);

 private:
  void build(const Mat &lImg, const Mat &rImg, int maxDis, Mat *vol, int right);
  int device_;
  bool fused_;
};
