/*
 * mjpeg-hip.cpp -- install as decoder/mjpeg-hip.cpp and add mjpeg-hip.o to decoder/Makefile.
 * Mirrors decoder/mjpeg-decoder-sw.cpp:95-142: `in` holds one MJPEG frame of at most `len` bytes,
 * `out` receives width x height x 3 bytes of RGB.  The frame is decoded on the device with
 * libjpeg's default methods (JDCT_ISLOW), not the JDCT_IFAST the software decoder asks for.
 */
#include "decoder/mjpeg-hip.h"

HIPMJPEGDecoder::HIPMJPEGDecoder(int maxWidth, int maxHeight)
{
	core = new rtdm::HIPMJPEGCore(maxWidth, maxHeight);
}

HIPMJPEGDecoder::~HIPMJPEGDecoder()
{
	delete core;
}

int HIPMJPEGDecoder::status() const
{
	return core->status();
}

int HIPMJPEGDecoder::decode(char* in, int len, int width, int height, char* out)
{
	if (len < 0)
		return RTDM_ERR_BAD_SIZE;
	return core->decode((const uint8_t*)in, (size_t)len, width, height, (uint8_t*)out);
}
