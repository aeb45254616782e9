function [worldPoints, reprojectionErrors, validIndex] = triangulate(matchedPoints1, matchedPoints2, cameraMatrix1, cameraMatrix2)
%TRIANGULATE libvo (MI355X) shadow: [worldPoints, reprojectionErrors, validIndex] = triangulate(x1, x2, P1, P2)
%   reference call sites: VO.m:113-116, CreateLandmarksFromFeatures.m:7.
%   x1, x2: N x 2 points (or point objects), P1, P2: 3 x 4 camera matrices
%   (VO.m:27-32).  Linear DLT per point in double, result returned as single
%   (VO.m passes single Locations).
%   reprojectionErrors: N x 1 single, the mean over the two views of the pixel
%   distance between a point and the reprojection of its worldPoints row.
%   validIndex: N x 1 logical, true where the point lies in front of both
%   cameras.  Both are computed from the single worldPoints returned (vo.h).
%   One output runs vo_triangulate alone, as before.
    if isobject(matchedPoints1), matchedPoints1 = matchedPoints1.Location; end
    if isobject(matchedPoints2), matchedPoints2 = matchedPoints2.Location; end
    P1 = double(cameraMatrix1);
    P2 = double(cameraMatrix2);
    if nargout > 2
        [worldPoints, reprojectionErrors, validIndex] = vo_mex('triangulate', matchedPoints1, matchedPoints2, P1, P2);
    elseif nargout > 1
        [worldPoints, reprojectionErrors] = vo_mex('triangulate', matchedPoints1, matchedPoints2, P1, P2);
    else
        worldPoints = vo_mex('triangulate', matchedPoints1, matchedPoints2, P1, P2);
    end
end
