// Surface loads through the C++ facade (tests/test_gpu_surface_facade.py):
//   --mode=source   LinElas on the unit cube with "Source Type" = "surface": writes the assembled source term
//   --mode=neumann  Laplace on the unit cube, u = 0 on flag 2 (x = 0), a "Neumann" entry of value --flux on flag 3 (x = 1)
//                   in the BCBuilder, no volume source: writes the solution
#include <cstring>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/problems/specific/Laplace.hpp"
#include "feddlib/problems/specific/LinElas.hpp"

using namespace FEDD;
typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

static double g_flux = 0.;
void zeroBC(double* x, double* res, double t, const double* parameters) { res[0] = 0.; }
void zeroBC3D(double* x, double* res, double t, const double* parameters) { res[0] = res[1] = res[2] = 0.; }
void fluxBC(double* x, double* res, double t, const double* parameters) { res[0] = g_flux; }
void noSource(double* x, double* res, double* parameters) { res[0] = 0.; }
// parameters = {time, force, loaded flag, flag of the element, degree}
void traction(double* x, double* res, double* parameters) {
    res[0] = parameters[3] == parameters[2] ? parameters[1] : 0.;
    res[1] = parameters[3] == parameters[2] ? -2. * parameters[1] : 0.;
    res[2] = 0.25 * parameters[3];
}

int main(int argc, char* argv[]) {
    Teuchos::GlobalMPISession mpiSession(&argc, &argv);
    std::string mode, problemFile, precFile, solverFile, outFile;
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        std::string tmp;
        if (val("mode", mode) || val("problemfile", problemFile) || val("precfile", precFile) || val("solverfile", solverFile) || val("out", outFile)) continue;
        if (val("flux", tmp)) { g_flux = std::atof(tmp.c_str()); continue; }
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::DefaultComm<int>::getComm();
        ParameterListPtr_Type all(new Teuchos::ParameterList(*Teuchos::getParametersFromXmlFile(problemFile)));
        all->setParameters(*Teuchos::getParametersFromXmlFile(precFile));
        all->setParameters(*Teuchos::getParametersFromXmlFile(solverFile));
        const int m = all->sublist("Parameter").get("H/h", 4);
        std::vector<double> x(3, 0.);
        Teuchos::RCP<Domain<SC, LO, GO, NO> > domain(new Domain<SC, LO, GO, NO>(x, 1., 1., 1., comm));
        domain->buildMesh(1, "Square", 3, "P1", 1, m, 0);
        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcFactory(new BCBuilder<SC, LO, GO, NO>());
        Teuchos::RCP<const MultiVector<SC, LO, GO, NO> > result;
        if (mode == "source") {
            bcFactory->addBC(zeroBC3D, 2, 0, domain, "Dirichlet", 3);
            LinElas<SC, LO, GO, NO> linElas(domain, "P1", all);
            linElas.addRhsFunction(traction);
            linElas.addBoundaries(bcFactory);
            linElas.addParemeterRhs(all->sublist("Parameter").get("Surface force", 0.));
            linElas.addParemeterRhs((double)all->sublist("Parameter").get("Surface Flag", 3));
            linElas.addParemeterRhs(0.);
            linElas.initializeProblem();
            linElas.assemble();
            result = linElas.getSourceTerm()->getBlock(0);
            std::ofstream out(outFile);
            out << std::setprecision(17);
            { auto data = result->getData(0); for (size_t i = 0; i < data.size(); ++i) out << data[i] << "\n"; }
        } else {
            bcFactory->addBC(zeroBC, 2, 0, domain, "Dirichlet", 1);
            bcFactory->addBC(fluxBC, 3, 0, domain, "Neumann", 1);
            Laplace<SC, LO, GO, NO> laplace(domain, "P1", all, false);
            laplace.addRhsFunction(noSource);
            laplace.addBoundaries(bcFactory);
            laplace.initializeProblem();
            laplace.assemble();
            laplace.setBoundaries();
            const int its = laplace.solve();
            std::cout << "iterations " << its << " relres " << laplace.getLastRelativeResidual() << std::endl;
            result = laplace.getSolution()->getBlock(0);
            std::ofstream out(outFile);
            out << std::setprecision(17);
            { auto data = result->getData(0); for (size_t i = 0; i < data.size(); ++i) out << data[i] << "\n"; }
        }
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
