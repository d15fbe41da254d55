// cuDiscreteLinearity.h -- drop-in header name of the reference (src/CuTNetLib/cuDiscreteLinearity.h): the MI355X CuTNetLib API lives in cudiscrete.h.
#pragma once
#include "../host/cudiscrete.h"
