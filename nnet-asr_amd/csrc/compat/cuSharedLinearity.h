// cuSharedLinearity.h -- drop-in header name of the reference (src/CuTNetLib/cuSharedLinearity.h): the MI355X CuTNetLib API lives in cushared.h.
#pragma once
#include "../host/cushared.h"
