/*
 * mjpeg-hip.h -- install as include/decoder/mjpeg-hip.h.  HIPMJPEGDecoder derives from the
 * reference's DecoderDevice (include/decoder/decoder.h:9-15) and stands where MJPEGDecoderDevice
 * (include/decoder/mjpeg-decoder-sw.h:19-28) stands; main.cpp:126 changes only the class name and
 * gains the frame size.  decoder.h carries no include guard: include this header AFTER estimator.h
 * (which brings mjpeg-decoder-sw.h and with it decoder.h), or on its own.
 */
#ifndef INCLUDE_DECODER_MJPEG_HIP_H_
#define INCLUDE_DECODER_MJPEG_HIP_H_

#ifndef INCLUDE_MJPEG_H_
#include "decoder/decoder.h"
#endif
#include "hip_matcher_core.h"

class HIPMJPEGDecoder: public DecoderDevice
{
public:
	/* the largest frame the cameras deliver (videoDev->getWidth() x getHeight()) */
	explicit HIPMJPEGDecoder(int maxWidth, int maxHeight);
	~HIPMJPEGDecoder();
	/* 0 on success, a negative rtdm_status otherwise (MJPEGDecoderDevice::decode returns 0 / -1) */
	int decode(char* in, int len, int width, int height, char* out);
	int status() const;
private:
	rtdm::HIPMJPEGCore* core;
};

#endif /* INCLUDE_DECODER_MJPEG_HIP_H_ */
