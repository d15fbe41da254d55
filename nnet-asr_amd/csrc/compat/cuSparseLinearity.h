// cuSparseLinearity.h -- drop-in header name of the reference (src/CuTNetLib/cuSparseLinearity.h): the MI355X CuTNetLib API lives in cusparse.h.
#pragma once
#include "../host/cusparse.h"
