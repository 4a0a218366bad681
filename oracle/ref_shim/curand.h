// TEST INFRASTRUCTURE -- the reference includes this header and uses nothing from it (see cuda_runtime.h here)
#pragma once
