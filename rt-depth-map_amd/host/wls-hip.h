/*
 * wls-hip.h -- install as include/stereo-matcher/wls-hip.h.  The reference's post-filter block (ENABLE_POST_FILTER,
 * estimator.cpp:57-70, include/estimator.h:32,116) calls cv::ximgproc::createRightMatcher, createDisparityWLSFilter and
 * DisparityWLSFilter::filter; these are the same calls over the device module.  The filter follows rules W1-W8 of
 * DESIGN.md section 4.9 (a restatement of ximgproc from memory: parity with the library is unpinned).  Frames must not be
 * larger than the left matcher's (width, height); the guide (left view) is CV_8UC1 or CV_8UC3.
 */
#ifndef INCLUDE_BM_WLS_HIP_H_
#define INCLUDE_BM_WLS_HIP_H_

#include "stereo-matcher/bm-hip.h"
#include "stereo-matcher/sgbm-hip.h"
#include "hip_matcher_core.h"

class HIPDisparityWLSFilter
{
public:
	explicit HIPDisparityWLSFilter(const rtdm::HIPMatcherCore& left);
	explicit HIPDisparityWLSFilter(const rtdm::HIPSGMCore& left);
	~HIPDisparityWLSFilter();
	/* ximgproc's argument order; returns 0 or a negative rtdm_status */
	int filter(cv::InputArray disparity_map_left, cv::InputArray left_view, cv::OutputArray filtered_disparity_map,
			cv::InputArray disparity_map_right);
	void setLambda(double lambda) { core->setLambda(lambda); }
	double getLambda() { return core->getLambda(); }
	void setSigmaColor(double sigma) { core->setSigmaColor(sigma); }
	double getSigmaColor() { return core->getSigmaColor(); }
	void setLRCthresh(int thresh) { core->setLRCthresh(thresh); }
	int getLRCthresh() { return core->getLRCthresh(); }
	void setDepthDiscontinuityRadius(int radius) { core->setDepthDiscontinuityRadius(radius); }
	int getDepthDiscontinuityRadius() { return core->getDepthDiscontinuityRadius(); }
	cv::Mat getConfidenceMap();
	cv::Rect getROI();
private:
	rtdm::HIPWLSCore* core;
	int rows, cols;
};

/* createRightMatcher / createDisparityWLSFilter for the HIP matchers; the caller deletes what they return */
HIPMatcher* createRightMatcher(HIPMatcher* left);
HIPSemiGlobalMatcher* createRightMatcher(HIPSemiGlobalMatcher* left);
HIPDisparityWLSFilter* createDisparityWLSFilter(HIPMatcher* left);
HIPDisparityWLSFilter* createDisparityWLSFilter(HIPSemiGlobalMatcher* left);

#endif /* INCLUDE_BM_WLS_HIP_H_ */
