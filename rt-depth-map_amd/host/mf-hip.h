/*
 * mf-hip.h -- install as include/filter/mf-hip.h.  HIPMorphologicalFilter derives from the
 * reference's VideoFilterDevice (include/filter/filter.h:13-37) with SWMorphologicalFilter's
 * constructor (include/filter/mf-sw.h:19-24); main.cpp:133 changes only the class name.
 */
#ifndef INCLUDE_FILTER_MF_HIP_H_
#define INCLUDE_FILTER_MF_HIP_H_

#include "filter/filter.h"
#include "hip_matcher_core.h"

class HIPMorphologicalFilter: public VideoFilterDevice
{
public:
	explicit HIPMorphologicalFilter(int w, int h, int bpp);
	~HIPMorphologicalFilter();
	int run(cv::InputArray in, cv::OutputArray out);
	/* beyond the reference's MORPH_FILTER_DX / MORPH_FILTER_DY: cv::getStructuringElement(shape, Size(width, height)) and
	 * cv::morphologyEx's operation (cv::MORPH_ERODE .. cv::MORPH_BLACKHAT, or RTDM_MORPH_OPEN_CLOSE, the default) from the
	 * next run on; an rtdm_status comes back. */
	int setElement(int shape, int width, int height);
	int setOperation(int op, int iterations = 1);
private:
	rtdm::HIPMorphCore* core;
};

#endif /* INCLUDE_FILTER_MF_HIP_H_ */
