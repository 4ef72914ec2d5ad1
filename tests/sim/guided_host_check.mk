# tests/sim/guided_host_check.mk -- TEST AID (never part of libmvo_hip.so, not run by the suite): guided_host_check.cpp with
# csrc/guided_match_host.h and hip_emu/, all under AddressSanitizer and UndefinedBehaviorSanitizer, as one program.
#   make -C tests/sim -f guided_host_check.mk check
include Makefile
_build/guided_host_check: guided_host_check.cpp $(CSRC)/guided_match_host.h hip_emu/emu_runtime.cpp $(CSRC)/mvo_internal.h hip_emu/hip/hip_runtime.h
	@mkdir -p _build
	$(CXX) $(FLAGS) -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ guided_host_check.cpp hip_emu/emu_runtime.cpp
check: _build/guided_host_check
	./_build/guided_host_check
.PHONY: check
