/*
 * xyz-hip.h -- install as include/stereo-matcher/xyz-hip.h.  The reference's two lines after the matcher (estimator.cpp:75-76),
 *     left_disp /= 16.;  reprojectImageTo3D(left_disp, xyz, Q, true, CV_32F);
 * as one call over the device module: pass the matcher's own CV_16SC1 x16 map (before the division; it is rounded half to
 * even inside, as `/= 16.` rounds it) and receive the CV_32FC3 xyz image calc_depth reads.  Rules X1-X8 of DESIGN.md section
 * 4.11 (a restatement of OpenCV from memory: parity with the library is unpinned).
 */
#ifndef INCLUDE_XYZ_HIP_H_
#define INCLUDE_XYZ_HIP_H_

#include <opencv2/opencv.hpp>
#include "hip_matcher_core.h"

/* Q: row-major 4x4 (for a CV_64F cv::Mat Q: (const double*) Q.data).  Returns 0 or a negative rtdm_status.  Keeps one device
 * handle between calls (re-made when a larger frame arrives), so call it from one thread, as Estimator::run does. */
int reprojectImageTo3D(cv::InputArray disparity, cv::OutputArray _3dImage, const double Q[16], bool handleMissingValues);

#endif /* INCLUDE_XYZ_HIP_H_ */
