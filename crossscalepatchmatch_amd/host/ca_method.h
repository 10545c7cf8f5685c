// ca_method.h -- cost-aggregation plugin interface, as CSPM/ca_method.h:8-25.  Implemented by BoxCA, GFCA and BFCA
// (ca_filter/device_ca.h, on the GPU); CSPatchMatch::LocalStereo runs the same filters inside the device cost object.
// PatchMatch itself never calls it, as in the reference.
#pragma once
#include "commfunc.h"

class CAMethod {
 public:
  CAMethod() {}
  virtual ~CAMethod() {}
  virtual void aggreCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol) = 0;
};
