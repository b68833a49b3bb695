# tests/cpp/row_softmax_sim.mk — TEST CODE: the one rule of row_softmax_sim, beside tests/cpp/Makefile (which it includes
# for CXX, CSRC, SIM_SAN, SIM_HDRS and sanitizer_probe).
#   row_softmax_sim   csrc/row_softmax.hip compiled UNCHANGED with the host compiler over simt/, with the address and
#                     undefined-behaviour sanitizers, and driven through mi355_spmv_row_softmax_create / _set_scale /
#                     _execute / _backward / _destroy: the program of tests/test_row_softmax_sim_cpu.py, built on demand
#                     by it:   make -C tests/cpp -f row_softmax_sim.mk row_softmax_sim
include Makefile

row_softmax_sim: row_softmax_sim.cpp $(CSRC)/row_softmax.hip $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<
