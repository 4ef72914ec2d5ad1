# host/tests/pose_optimization.mk -- test_pose_optimization: the mirror of the robust motion-only pose optimisation
# (my_slam/vo/pose_optimization.h), written against the reference-shaped headers and linked to libmvo_hip.so only
# (tests/test_pose_optimization_host.py runs it on the MI355X and, with the emulated build in front of the library search path, on
# the CPU).
#   make -C host/tests -f pose_optimization.mk
include Makefile
pose_optimization: test_pose_optimization
test_pose_optimization: test_pose_optimization.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_pose_optimization.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := pose_optimization
.PHONY: pose_optimization
