// device_ca.h -- the reference's three CAMethod implementations (CSPM/ca_filter/BoxCA.h, GFCA.h, BFCA.h): aggreCV filters the
// slices 1 .. maxDis-1 of costVol in place, guided by lImg exactly as given (rImg is unused), with the HIP kernels of
// libcspm_hip.so (cspm_aggregate_cv_host) on the GPU of the calling thread's DeviceSlot.  lImg must be CV_64FC3 (the colour
// branch: gray guides are not supported) and every slice CV_64FC1 of lImg's size; anything else throws, like GrdCC.
#pragma once
#include "../../../include/cspm.h"
#include "../ca_method.h"

class DeviceCA : public CAMethod {
 public:
  explicit DeviceCA(int method) : method_(method) {}
  void aggreCV(const Mat &lImg, const Mat &rImg, const int maxDis, Mat *costVol);

 private:
  int method_;  // CSPM_CA_*
};

class BoxCA : public DeviceCA {  // BoxFilter(costVol[d], 3): the unnormalised 7x7 sum (BoxCA.cpp:5-13)
 public:
  BoxCA() : DeviceCA(CSPM_CA_BOX) {}
};
class GFCA : public DeviceCA {  // GuidedFilter(lImg, costVol[d]): r = 9, eps = 0.0001f (GFCA.cpp:5-12)
 public:
  GFCA() : DeviceCA(CSPM_CA_GF) {}
};
class BFCA : public DeviceCA {  // BilateralFilter(lImg, costVol[d], 35) (BFCA.cpp:5-13)
 public:
  BFCA() : DeviceCA(CSPM_CA_BF) {}
};
