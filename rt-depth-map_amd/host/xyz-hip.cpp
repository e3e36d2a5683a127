/*
 * xyz-hip.cpp -- install as stereo-matcher/xyz-hip.cpp and add xyz-hip.o to stereo-matcher/Makefile.
 * cv::reprojectImageTo3D's call shape over HIPXYZCore.
 */
#include "stereo-matcher/xyz-hip.h"

int reprojectImageTo3D(cv::InputArray disparity, cv::OutputArray _3dImage, const double Q[16], bool handleMissingValues)
{
	static rtdm::HIPXYZCore* core = nullptr;
	cv::Mat d = disparity.getMat();
	if (d.type() != CV_16SC1 || d.empty())
		return RTDM_ERR_BAD_SIZE;
	if (!core || !core->handle() || d.cols > core->maxWidth() || d.rows > core->maxHeight()) {
		delete core;
		/* a core whose construction failed (no handle) is made again; min_disparity is read by the cloud only */
		core = new rtdm::HIPXYZCore(Q, d.cols, d.rows, 0, RTDM_XYZ_ROUNDED, handleMissingValues);
	}
	int rc = core->setQ(Q);
	if (rc == RTDM_OK)
		rc = core->setHandleMissingValues(handleMissingValues);
	if (rc != RTDM_OK)
		return rc;
	_3dImage.create(d.size(), CV_32FC3);
	cv::Mat o = _3dImage.getMat();
	return core->reprojectImageTo3D((const int16_t*) d.data, d.step, d.rows, d.cols, (float*) o.data, o.step);
}
