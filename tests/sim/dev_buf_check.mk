# tests/sim/dev_buf_check.mk -- TEST AID (never part of libmvo_hip.so): dev_buf_check.cpp with DevBuf of csrc/mvo_internal.h and
# hip_emu/, all under AddressSanitizer (with its leak check) and UndefinedBehaviorSanitizer, as one program.
#   make -C tests/sim -f dev_buf_check.mk check
include Makefile
_build/dev_buf_check: dev_buf_check.cpp hip_emu/emu_runtime.cpp $(CSRC)/mvo_internal.h hip_emu/hip/hip_runtime.h
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ dev_buf_check.cpp hip_emu/emu_runtime.cpp
check: _build/dev_buf_check
	./_build/dev_buf_check
.PHONY: check
