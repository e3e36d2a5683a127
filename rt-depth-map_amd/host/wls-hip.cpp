/*
 * wls-hip.cpp -- install as stereo-matcher/wls-hip.cpp and add wls-hip.o to stereo-matcher/Makefile.
 * The ximgproc call shapes over HIPWLSCore; the matchers' cores are reached through HIPMatcher::getCore /
 * HIPSemiGlobalMatcher::getCore.
 */
#include "stereo-matcher/wls-hip.h"

HIPDisparityWLSFilter::HIPDisparityWLSFilter(const rtdm::HIPMatcherCore& left)
	: core(new rtdm::HIPWLSCore(left)), rows(0), cols(0) {}

HIPDisparityWLSFilter::HIPDisparityWLSFilter(const rtdm::HIPSGMCore& left)
	: core(new rtdm::HIPWLSCore(left)), rows(0), cols(0) {}

HIPDisparityWLSFilter::~HIPDisparityWLSFilter()
{
	delete core;
}

int HIPDisparityWLSFilter::filter(cv::InputArray disparity_map_left, cv::InputArray left_view,
		cv::OutputArray filtered_disparity_map, cv::InputArray disparity_map_right)
{
	cv::Mat l = disparity_map_left.getMat(), g = left_view.getMat(), r = disparity_map_right.getMat();
	if (l.type() != CV_16SC1 || (g.type() != CV_8UC1 && g.type() != CV_8UC3) || g.size() != l.size())
		return RTDM_ERR_BAD_SIZE;
	const bool right = !r.empty();
	if (right && (r.type() != CV_16SC1 || r.size() != l.size()))
		return RTDM_ERR_BAD_SIZE;
	filtered_disparity_map.create(l.size(), CV_16SC1);
	cv::Mat o = filtered_disparity_map.getMat();
	rows = l.rows; cols = l.cols;
	return core->filter((const int16_t*) l.data, l.step, g.data, g.step, g.channels(), l.rows, l.cols, (int16_t*) o.data,
			o.step, right ? (const int16_t*) r.data : nullptr, right ? r.step : 0);
}

cv::Mat HIPDisparityWLSFilter::getConfidenceMap()
{
	/* a view of the core's buffer, valid until the next filter call (ximgproc also returns its member) */
	return cv::Mat(rows, cols, CV_32FC1, (void*) core->confidenceMap());
}

cv::Rect HIPDisparityWLSFilter::getROI()
{
	const rtdm::Rect r = core->roi(rows, cols);
	return cv::Rect(r.x, r.y, r.width, r.height);
}

HIPMatcher* createRightMatcher(HIPMatcher* left)
{
	return new HIPMatcher(rtdm::createRightMatcher(*left->getCore()));
}

HIPSemiGlobalMatcher* createRightMatcher(HIPSemiGlobalMatcher* left)
{
	return new HIPSemiGlobalMatcher(rtdm::createRightMatcher(*left->getCore()));
}

HIPDisparityWLSFilter* createDisparityWLSFilter(HIPMatcher* left)
{
	return new HIPDisparityWLSFilter(*left->getCore());
}

HIPDisparityWLSFilter* createDisparityWLSFilter(HIPSemiGlobalMatcher* left)
{
	return new HIPDisparityWLSFilter(*left->getCore());
}
