// Test program for the interface side of the facade (tests/test_gpu_geometry_laplace_facade.py), one rank:
//   --mode=mismatch   identifyInterfaceParallelAndDistance against a domain with another number of interface nodes
//   --mode=foreign    FE::assemblyLaplaceXDim with a function that is not HeuristicScaling
//   --mode=nodist     FE::assemblyLaplaceXDim, calculateDistancesToInterface and getDistancesToInterface on a domain without an interface
//   --mode=distances  identify on flag 2, get, set(get) and print the distances by local repeated id
// Each error mode prints what() of the exception it caught and returns 0; it returns 3 if nothing was thrown.
#include <iomanip>
#include <iostream>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/FE/FE.hpp"

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;
using namespace FEDD;

static double otherScaling(double* x, double* p) { return x[0] <= p[0] ? p[1] : 1.0; }     // <= where HeuristicScaling has <

static Teuchos::RCP<Domain<SC, LO, GO, NO> > square(Teuchos::RCP<const Teuchos::Comm<int> > comm, int m) {
    std::vector<double> x(2, 0.0);
    Teuchos::RCP<Domain<SC, LO, GO, NO> > d(new Domain<SC, LO, GO, NO>(x, 1., 1., comm));
    d->buildMesh(1, "Square", 2, "P1", 1, m, 0);
    return d;
}

int main(int argc, char* argv[]) {
    Teuchos::GlobalMPISession mpiSession(&argc, &argv);
    std::string mode;
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        if (a.compare(0, 7, "--mode=") == 0) mode = a.substr(7);
    }
    Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::DefaultComm<int>::getComm();
    try {
        auto domain = square(comm, 4);
        typedef Matrix<SC, LO, GO, NO> Matrix_Type;
        Teuchos::RCP<Matrix_Type> H(new Matrix_Type(domain->getMapVecFieldUnique(), 2 * domain->getApproxEntriesPerRow()));
        FE<SC, LO, GO, NO> fe;
        fe.addFE(domain);
        double parameter[2] = {0.3, 50.};
        if (mode == "mismatch") {
            auto other = square(comm, 6);
            vec_int_Type flags(1, 2);
            try {
                domain->identifyInterfaceParallelAndDistance(other, flags);
            } catch (const std::exception& e) {
                std::cout << "caught: " << e.what() << std::endl;
                std::cout << "has distances " << domain->hasDistancesToInterface() << std::endl;
                return 0;
            }
            return 3;
        }
        if (mode == "foreign") {
            vec_int_Type flags(1, 2);
            domain->identifyInterfaceParallelAndDistance(domain, flags);
            try {
                fe.assemblyLaplaceXDim(2, "P1", H, otherScaling, parameter);
            } catch (const std::exception& e) {
                std::cout << "caught: " << e.what() << std::endl;
                fe.assemblyLaplaceXDim(2, "P1", H, HeuristicScaling, parameter);     // the reference's function is taken
                std::cout << "HeuristicScaling accepted" << std::endl;
                return 0;
            }
            return 3;
        }
        if (mode == "nodist") {
            int caught = 0;
            try {
                fe.assemblyLaplaceXDim(2, "P1", H, HeuristicScaling, parameter);
            } catch (const std::exception& e) {
                std::cout << "caught assembly: " << e.what() << std::endl;
                ++caught;
            }
            try {
                domain->calculateDistancesToInterface();
            } catch (const std::exception& e) {
                std::cout << "caught calculate: " << e.what() << std::endl;
                ++caught;
            }
            try {
                domain->getDistancesToInterface();
            } catch (const std::exception& e) {
                std::cout << "caught get: " << e.what() << std::endl;
                ++caught;
            }
            return caught == 3 ? 0 : 3;
        }
        if (mode == "distances") {
            vec_int_Type flags(1, 2);
            domain->identifyInterfaceParallelAndDistance(domain, flags);
            vec_dbl_ptr_Type d = domain->getDistancesToInterface();
            domain->setDistancesToInterface(d);
            vec_dbl_ptr_Type d2 = domain->getDistancesToInterface();
            domain->calculateDistancesToInterface();
            vec_dbl_ptr_Type d3 = domain->getDistancesToInterface();
            if (*d != *d2 || *d != *d3) return 4;
            auto pts = domain->getPointsRepeated();
            std::cout << std::setprecision(17);
            for (size_t i = 0; i < d->size(); ++i) std::cout << "dist " << i << " " << (*pts)[i][0] << " " << (*pts)[i][1] << " " << (*d)[i] << "\n";
            return 0;
        }
        std::cerr << "unknown mode " << mode << std::endl;
        return 2;
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
}
