/*
 * sgbm-hip.h -- install as include/stereo-matcher/sgbm-hip.h.  HIPSemiGlobalMatcher derives from the reference's
 * BlockMatcher with SWSemiGlobalMatcher's constructor (include/stereo-matcher/sgbm-sw.h:27-28) plus the frame size.
 * Like SWSemiGlobalMatcher it is not selected by main.cpp unless the maintainer does so.  The device module runs
 * cv::StereoSGBM's MODE_SGBM (or, by the trailing mode argument, MODE_HH or MODE_HH4; MODE_SGBM_3WAY is refused there and served by setMode) as restated in oracle/sgm_oracle.c (bit-exact against that restatement; against the
 * library itself parity is unpinned); numOfDisparities is any multiple of 16, as in the library (checked by the device module,
 * not here; above 256 the path passes run on its wide-line kernel); an even blockSize runs as the next odd one (as in the library); where a window is large enough, a frame whose block cost + P2 would pass 32767 (where the library's 16-bit costs wrap) makes compute return an error.
 * compute takes CV_8UC1 or CV_8UC3 pairs and setPreFilterCap takes 0 .. 127, as cv::StereoSGBM does (the colour pixel cost
 * restates the library's from memory; parity unpinned).
 */
#ifndef INCLUDE_BM_SGBM_HIP_H_
#define INCLUDE_BM_SGBM_HIP_H_

#include "stereo-matcher/stereo-matcher.h"
#include "hip_matcher_core.h"

class HIPSemiGlobalMatcher: public BlockMatcher
{
public:
	HIPSemiGlobalMatcher(int blockSize, int minDisparity, int numOfDisparities, int uniquenessRatio,
			int speckleWindowSize, int speckleRange, int disp12MaxDiff, int width, int height,
			int mode = rtdm::MODE_SGBM /* cv::StereoSGBM::setMode: MODE_SGBM, MODE_HH, MODE_HH4 */);
	~HIPSemiGlobalMatcher();
	int compute(cv::InputArray left, cv::InputArray right, cv::OutputArray out);
	int setPreFilterCap(int preFilterCap) { return core->setPreFilterCap(preFilterCap); }
	/* RTDM_SGM_COST_BT (the library's cost, the default) or RTDM_SGM_COST_CENSUS over a cw x ch window: for two cameras with
	 * their own auto-exposure; not a cv::StereoSGBM feature (include/rtdm.h, rtdm_sgm_set_cost).  CV_8UC1 pairs only. */
	int setCost(int cost, int cw = 9, int ch = 7) { return core->setCost(cost, cw, ch); }
	/* cv::StereoSGBM::setMode on the live matcher, from the next compute on: rtdm::MODE_SGBM, MODE_HH, MODE_HH4 or
	 * MODE_SGBM_3WAY -- the one door to the last (include/rtdm.h, rtdm_sgm_set_mode; numOfDisparities <= 256) */
	int setMode(int mode) { return core->setMode(mode); }
	int getMode() const { return core->mode(); }
	void setROI1(cv::Rect roi1) {}
	void setROI2(cv::Rect roi2) {}
	/* takes ownership of a core (createRightMatcher, wls-hip.cpp) */
	explicit HIPSemiGlobalMatcher(rtdm::HIPSGMCore* core) : core(core) {}
	rtdm::HIPSGMCore* getCore() { return core; }
private:
	rtdm::HIPSGMCore* core;
};

#endif /* INCLUDE_BM_SGBM_HIP_H_ */
