# host/tests/orb_distribute.mk -- test_orb_distribute: the mirror of the cell-wise detector (my_slam/geometry/orb_distribute.h)
# and the Frame::calcKeyPoints that can use it, written against the reference-shaped headers and linked to libmvo_hip.so only
# (tests/test_orb_distribute_host.py runs it on the MI355X and, with the emulated build in front of the library search path,
# on the CPU).
#   make -C host/tests -f orb_distribute.mk
include Makefile
orb_distribute: test_orb_distribute
test_orb_distribute: test_orb_distribute.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_orb_distribute.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := orb_distribute
.PHONY: orb_distribute
