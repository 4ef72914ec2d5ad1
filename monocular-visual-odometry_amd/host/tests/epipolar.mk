# host/tests/epipolar.mk -- test_epipolar_match: the mirror of the pose-guided matcher and the keyframe insertion that can use
# it, written against the reference-shaped headers and linked to libmvo_hip.so only (tests/test_epipolar_host.py runs it on
# the MI355X and, with the emulated build in front of the library search path, on the CPU).
#   make -C host/tests -f epipolar.mk
include Makefile
epipolar: test_epipolar_match
test_epipolar_match: test_epipolar_match.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_epipolar_match.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := epipolar
.PHONY: epipolar
